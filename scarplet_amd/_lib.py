"""ctypes binding of libscarplet_hip.so (include/scarplet_hip.h).

The library is the only compute path: if it cannot be loaded, or no GPU is
visible, the matcher raises - there is no CPU fallback in this package.
"""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCARPLET_HIP_LIB is the ONE environment variable this package reads: a developer hook of the
# tools/ scripts to load another build of the same library (tools/build_alt.sh).  The engine
# itself - libscarplet_hip.so - reads no environment at all; its options go through
# sc_set_option.
LIB_PATH = os.environ.get("SCARPLET_HIP_LIB") or os.path.join(_HERE, "libscarplet_hip.so")

SC_OK = 0
SC_ERR_INVALID = -1
ABI_VERSION = 10
ID_NONE = 0xFFFFFFFF
COMM_ID_BYTES = 128
KIND_WINDOW = 2             # SC_KIND_WINDOW: a template whose window the host uploaded (sc_upload_window)

K_NAMES = ("k_curv", "k_windows", "k_direct", "k_fwd_rows", "k_fwd_cols",
           "k_inv_cols", "k_inv_rows", "k_settle", "k_noise", "k_trace", "k_profile")
(K_CURV, K_WINDOWS, K_DIRECT, K_FWD_ROWS, K_FWD_COLS, K_INV_COLS, K_INV_ROWS, K_SETTLE, K_NOISE, K_TRACE,
 K_PROFILE) = range(11)
NOISE_MAX_RADIUS = 1048576  # SC_NOISE_MAX_RADIUS: the largest filter radius sc_curvature_noise takes

XFER_RECV, XFER_SEND, XFER_LOCAL = 0, 1, 2


class ScarpletHipError(RuntimeError):
    pass


def is_settle_limit(err):
    """Whether ``err`` is a float64 settle that stopped at one of its bounds - an overflowed event list, more float64
    work than it was allowed - rather than failed: the float32 record it left stands."""
    msg = str(err)
    return "overflowed" in msg or "too much float64 work" in msg


class sc_template(C.Structure):
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32),
                ("cos_a", C.c_double), ("sin_a", C.c_double),
                ("c", C.c_double), ("d", C.c_double),
                ("p0", C.c_double), ("p1", C.c_double),
                ("cc", C.c_double), ("sc2", C.c_double), ("ss", C.c_double),
                ("ilo", C.c_int32), ("ihi", C.c_int32),
                ("jlo", C.c_int32), ("jhi", C.c_int32),
                ("pmin", C.c_int32), ("pmax", C.c_int32),
                ("qmin", C.c_int32), ("qmax", C.c_int32),
                ("id", C.c_uint32), ("window", C.c_int32)]


class sc_plan(C.Structure):
    _fields_ = [("method", C.c_int32), ("Ty", C.c_int32), ("Tx", C.c_int32),
                ("Vy", C.c_int32), ("Vx", C.c_int32), ("nty", C.c_int32),
                ("ntx", C.c_int32), ("circ_y", C.c_int32),
                ("circ_x", C.c_int32), ("Py", C.c_int32), ("Qx", C.c_int32),
                ("group", C.c_int32)]


class sc_segment(C.Structure):
    """One row of the table of sc_trace_planes / sc_trace_result (docs/traces.md)."""
    _fields_ = [("first", C.c_int64), ("n_cells", C.c_int64), ("n_strong", C.c_int64),
                ("row_min", C.c_int32), ("row_max", C.c_int32), ("col_min", C.c_int32), ("col_max", C.c_int32),
                ("peak", C.c_int64),
                ("snr_peak", C.c_double), ("amp_peak", C.c_double), ("age_peak", C.c_double), ("angle_peak", C.c_double),
                ("sum_amp", C.c_double), ("sum_abs_amp", C.c_double), ("sum_age", C.c_double), ("sum_snr", C.c_double),
                ("sum_cos2a", C.c_double), ("sum_sin2a", C.c_double)]


# the same layout as a numpy structured dtype (the table is copied into such an array): here and below numpy derives
# names, formats, offsets and itemsize from the Structure itself
SEGMENT_DTYPE = np.dtype(sc_segment)


class sc_profile_fit(C.Structure):
    """One row of sc_fit_profiles / sc_fit_profiles_dem (docs/profiles.md)."""
    _fields_ = [("cell", C.c_int64), ("n", C.c_int32), ("kt_index", C.c_int32), ("lo_index", C.c_int32),
                ("hi_index", C.c_int32), ("status", C.c_int32),
                ("kt", C.c_double), ("kt_lo", C.c_double), ("kt_hi", C.c_double),
                ("a", C.c_double), ("b", C.c_double), ("c0", C.c_double), ("sse", C.c_double), ("rmse", C.c_double)]


PROFILE_DTYPE = np.dtype(sc_profile_fit)
PROFILE_MAX_AGES, PROFILE_MAX_HALF, PROFILE_MAX_SWATH = 64, 1024, 32   # SC_PROFILE_MAX_*
PROFILE_MAX_SHIFT = 64                                                 # SC_PROFILE_MAX_SHIFT


class sc_profile_shift_fit(C.Structure):
    """One row of sc_fit_profiles_shift / sc_fit_profiles_shift_dem: sc_profile_fit and the shift of the best age."""
    _fields_ = sc_profile_fit._fields_ + [("shift_index", C.c_int32), ("shift", C.c_double)]


PROFILE_SHIFT_DTYPE = np.dtype(sc_profile_shift_fit)
CHANNEL_MAX_FREQS = 64                                                 # SC_CHANNEL_MAX_FREQS (the rows of sc_channel_profiles are these)


class sc_profile_robust_fit(C.Structure):
    """One row of sc_fit_profiles_robust / sc_fit_profiles_robust_dem: sc_profile_fit, then the loss and the scale."""
    _fields_ = sc_profile_fit._fields_ + [("loss", C.c_double), ("scale", C.c_double), ("n_down", C.c_int32),
                                          ("ls_index", C.c_int32)]


PROFILE_ROBUST_DTYPE = np.dtype(sc_profile_robust_fit)
ROBUST_NONE, ROBUST_HUBER, ROBUST_TUKEY = 0, 1, 2                      # SC_ROBUST_*
ROBUST_MAX_ITER = 64                                                   # SC_ROBUST_MAX_ITER


class sc_profile_ramp_fit(C.Structure):
    """One row of sc_fit_profiles_ramp / sc_fit_profiles_ramp_dem: sc_profile_fit, then the half-width of the best age."""
    _fields_ = sc_profile_fit._fields_ + [("width_index", C.c_int32), ("width", C.c_double), ("initial_slope", C.c_double)]


PROFILE_RAMP_DTYPE = np.dtype(sc_profile_ramp_fit)
PROFILE_MAX_WIDTH = 64                                                 # SC_PROFILE_MAX_WIDTH
RAMP_FREE, RAMP_SLOPE = 0, 1                                           # SC_RAMP_*


FINE_FLOATS = ("kt_fine", "kt_lo_fine", "kt_hi_fine", "a_fine", "b_fine", "c0_fine", "sse_fine", "rmse_fine", "height_fine")


class sc_profile_fine_fit(C.Structure):
    """One row of sc_fit_profiles_refine / sc_fit_profiles_refine_dem: sc_profile_fit, then the minimum and the interval off
    the grid (docs/profiles.md, "Continuous ages")."""
    _fields_ = sc_profile_fit._fields_ + [(f, C.c_double) for f in FINE_FLOATS] + [("status_fine", C.c_int32)]


PROFILE_FINE_DTYPE = np.dtype(sc_profile_fine_fit)
PROFILE_MAX_REFINE = 2                                                 # SC_PROFILE_MAX_REFINE


class sc_segment_fit(C.Structure):
    """One row of sc_fit_segments / sc_fit_segments_dem (docs/segments.md)."""
    _fields_ = [("label", C.c_int32), ("n_cells", C.c_int32), ("n_profiles", C.c_int32), ("n", C.c_int32),
                ("dof", C.c_int32), ("kt_index", C.c_int32), ("lo_index", C.c_int32), ("hi_index", C.c_int32),
                ("status", C.c_int32),
                ("kt", C.c_double), ("kt_lo", C.c_double), ("kt_hi", C.c_double),
                ("a", C.c_double), ("sse", C.c_double), ("rmse", C.c_double)]


class sc_segment_cell(C.Structure):
    """One cell of the cell table of sc_fit_segments / sc_fit_segments_dem."""
    _fields_ = [("cell", C.c_int64), ("used", C.c_int32), ("n", C.c_int32),
                ("b", C.c_double), ("c0", C.c_double), ("sse", C.c_double)]


SEGMENT_FIT_DTYPE = np.dtype(sc_segment_fit)
SEGMENT_CELL_DTYPE = np.dtype(sc_segment_cell)
SEGMENT_MAX_PARK = 1 << 32                                             # SC_SEGMENT_MAX_PARK


class sc_segment_shift_cell(C.Structure):
    """One cell of the cell table of sc_fit_segments_shift / sc_fit_segments_shift_dem."""
    _fields_ = sc_segment_cell._fields_ + [("shift_index", C.c_int32)]


SEGMENT_SHIFT_CELL_DTYPE = np.dtype(sc_segment_shift_cell)


class sc_channel_segment_cell(C.Structure):
    """One cell of the cell table of sc_channel_segments / sc_channel_segments_dem (docs/channels.md)."""
    _fields_ = [("cell", C.c_int64), ("used", C.c_int32), ("n", C.c_int32),
                ("a", C.c_double), ("b", C.c_double), ("c0", C.c_double), ("sse", C.c_double), ("shift_index", C.c_int32)]


CHANNEL_SEGMENT_CELL_DTYPE = np.dtype(sc_channel_segment_cell)
CHANNEL_DEPTH_PROFILE, CHANNEL_DEPTH_SEGMENT = 0, 1                    # SC_CHANNEL_DEPTH_*


def channel_segment_park(h, n_freqs):
    """SC_CHANNEL_SEGMENT_PARK: the bytes sc_channel_segments parks per cell, in both modes."""
    return 8 * ((2 * h + 1) + 4 * n_freqs) + n_freqs


def channel_segment_cap(h, n_freqs):
    """The cells of one reach the park of sc_channel_segments holds."""
    return SEGMENT_MAX_PARK // channel_segment_park(h, n_freqs)


class sc_channel_boot(C.Structure):
    """One row of sc_channel_bootstrap / sc_channel_bootstrap_dem (docs/channels.md, "Intervals per reach")."""
    _fields_ = [("label", C.c_int32), ("n_cells", C.c_int32), ("n_profiles", C.c_int32), ("n_blocks", C.c_int32),
                ("replicates", C.c_int32), ("n_failed", C.c_int32), ("f_index0", C.c_int32), ("lo_index", C.c_int32),
                ("hi_index", C.c_int32), ("status", C.c_int32),
                ("f0", C.c_double), ("f_lo", C.c_double), ("f_hi", C.c_double), ("a0", C.c_double),
                ("a_mean", C.c_double), ("a_sd", C.c_double), ("a_lo", C.c_double), ("a_hi", C.c_double),
                ("area0", C.c_double), ("area_mean", C.c_double), ("area_sd", C.c_double), ("area_lo", C.c_double),
                ("area_hi", C.c_double)]


CHANNEL_BOOT_DTYPE = np.dtype(sc_channel_boot)


class sc_segment_ramp_fit(C.Structure):
    """One row of sc_fit_segments_ramp / sc_fit_segments_ramp_dem: sc_segment_fit, then the half-width of the best age."""
    _fields_ = sc_segment_fit._fields_ + [("width_index", C.c_int32), ("width", C.c_double), ("initial_slope", C.c_double)]


SEGMENT_RAMP_FIT_DTYPE = np.dtype(sc_segment_ramp_fit)


class sc_segment_robust_fit(C.Structure):
    """One row of sc_fit_segments_robust / sc_fit_segments_robust_dem: sc_segment_fit, then the loss and the scale."""
    _fields_ = sc_segment_fit._fields_ + [("loss", C.c_double), ("scale", C.c_double), ("n_down", C.c_int32),
                                          ("ls_index", C.c_int32), ("n_dormant", C.c_int32)]


class sc_segment_robust_cell(C.Structure):
    """One cell of the cell table of sc_fit_segments_robust / sc_fit_segments_robust_dem."""
    _fields_ = sc_segment_cell._fields_ + [("loss", C.c_double), ("n_down", C.c_int32), ("dormant", C.c_int32)]


SEGMENT_ROBUST_FIT_DTYPE = np.dtype(sc_segment_robust_fit)
SEGMENT_ROBUST_CELL_DTYPE = np.dtype(sc_segment_robust_cell)
SEGMENT_ROBUST_PLANES = 9                                              # SC_SEGMENT_ROBUST_PLANES


SEGMENT_FINE_FLOATS = ("kt_fine", "kt_lo_fine", "kt_hi_fine", "a_fine", "sse_fine", "rmse_fine")
SEGMENT_FINE_CELL_FLOATS = ("b_fine", "c0_fine", "sse_fine")


class sc_segment_fine_fit(C.Structure):
    """One row of sc_fit_segments_refine / sc_fit_segments_refine_dem: sc_segment_fit, then the minimum and the interval off
    the grid (docs/segments.md, "Continuous ages")."""
    _fields_ = sc_segment_fit._fields_ + [(f, C.c_double) for f in SEGMENT_FINE_FLOATS] + [("status_fine", C.c_int32)]


class sc_segment_fine_cell(C.Structure):
    """One cell of the cell table of sc_fit_segments_refine / sc_fit_segments_refine_dem."""
    _fields_ = sc_segment_cell._fields_ + [(f, C.c_double) for f in SEGMENT_FINE_CELL_FLOATS]


SEGMENT_FINE_FIT_DTYPE = np.dtype(sc_segment_fine_fit)
SEGMENT_FINE_CELL_DTYPE = np.dtype(sc_segment_fine_cell)
SEGMENT_REFINE_COLUMNS = 128                                           # SC_SEGMENT_REFINE_COLUMNS


def segment_refine_cap(h, n_ages, refine):
    """The cells of one segment the park of sc_fit_segments_refine holds: 8 ((2h + 1) + 4 (A + Cc)) bytes a cell, Cc the 128
    candidate columns of a round (none with ``refine`` 0)."""
    return SEGMENT_MAX_PARK // (8 * ((2 * h + 1) + 4 * (n_ages + (SEGMENT_REFINE_COLUMNS if refine > 0 else 0))))


def segment_robust_cap(h, n_ages, plane):
    """The cells of one segment the park of sc_fit_segments_robust holds: 8 ((2h + 1)(1 + plane) + 9 A) bytes a cell."""
    return SEGMENT_MAX_PARK // (8 * ((2 * h + 1) * (2 if plane else 1) + SEGMENT_ROBUST_PLANES * n_ages))


class sc_segment_boot(C.Structure):
    """One row of sc_bootstrap_segments / sc_bootstrap_segments_dem (docs/bootstrap.md)."""
    _fields_ = [("label", C.c_int32), ("n_cells", C.c_int32), ("n_profiles", C.c_int32), ("n_blocks", C.c_int32),
                ("replicates", C.c_int32), ("n_failed", C.c_int32), ("kt_index0", C.c_int32), ("lo_index", C.c_int32),
                ("hi_index", C.c_int32), ("status", C.c_int32),
                ("kt0", C.c_double), ("kt_lo", C.c_double), ("kt_hi", C.c_double), ("a0", C.c_double),
                ("a_mean", C.c_double), ("a_sd", C.c_double), ("a_lo", C.c_double), ("a_hi", C.c_double)]


SEGMENT_BOOT_DTYPE = np.dtype(sc_segment_boot)
BOOT_MAX_REPLICATES = 4096                                             # SC_BOOT_MAX_REPLICATES


class sc_strike_fit(C.Structure):
    """One row of sc_fit_strike / sc_fit_strike_dem (docs/strike.md)."""
    _fields_ = [("label", C.c_int32), ("station", C.c_int32), ("n_cells", C.c_int32), ("n_profiles", C.c_int32),
                ("n", C.c_int32), ("dof", C.c_int32), ("kt_index", C.c_int32), ("lo_index", C.c_int32),
                ("hi_index", C.c_int32), ("status", C.c_int32),
                ("kt", C.c_double), ("kt_lo", C.c_double), ("kt_hi", C.c_double),
                ("a", C.c_double), ("sse", C.c_double), ("rmse", C.c_double)]


STRIKE_FIT_DTYPE = np.dtype(sc_strike_fit)


class sc_strike_boot(C.Structure):
    """One row of sc_strike_bootstrap / sc_strike_bootstrap_dem (docs/strike.md, "Intervals per station")."""
    _fields_ = [("label", C.c_int32), ("station", C.c_int32), ("n_cells", C.c_int32), ("n_profiles", C.c_int32),
                ("n_blocks", C.c_int32), ("replicates", C.c_int32), ("n_failed", C.c_int32), ("kt_index0", C.c_int32),
                ("lo_index", C.c_int32), ("hi_index", C.c_int32), ("status", C.c_int32),
                ("kt0", C.c_double), ("kt_lo", C.c_double), ("kt_hi", C.c_double), ("a0", C.c_double),
                ("a_mean", C.c_double), ("a_sd", C.c_double), ("a_lo", C.c_double), ("a_hi", C.c_double)]


STRIKE_BOOT_DTYPE = np.dtype(sc_strike_boot)
STRIKE_BOOT_LDS_TERMS = 65536                                          # SB_LDS_TERMS of sc_strike_bootstrap.hip


class sc_channel_strike_boot(C.Structure):
    """One row of sc_channel_strike_bootstrap / sc_channel_strike_bootstrap_dem (docs/channels.md, "Intervals per station"):
    sc_channel_boot with the station."""
    _fields_ = sc_channel_boot._fields_[:1] + [("station", C.c_int32)] + sc_channel_boot._fields_[1:]


CHANNEL_STRIKE_BOOT_DTYPE = np.dtype(sc_channel_strike_boot)
CHANNEL_STRIKE_BOOT_LDS_TERMS = 65536                                  # CWB_LDS_TERMS of sc_channel_strike_bootstrap.hip
LDS_BYTES = 160 * 1024                                                 # a workgroup's LDS on gfx950
CHANNEL_STRIKE_BOOT_LDS_STATIC = 288                                   # k_cwb_window's own: the histogram, the counts, replicate 0


def channel_strike_boot_lds(n_blocks, n_freqs, replicates, profile_mode):
    """The dynamic LDS of k_cwb_window for a window of ``n_blocks`` blocks (cwb_lds_bytes, sc_channel_strike_bootstrap.hip):
    the block terms, two arrays of doubles padded to the sort, m_b in profile mode, the indices."""
    p2 = 2
    while p2 < replicates:
        p2 <<= 1
    return 16 * n_blocks * n_freqs + 17 * p2 + (4 * n_blocks if profile_mode else 0)


# the top of the accepted range - 64 KiB of terms at F = 1, R = 4096, profile mode - fits a workgroup: 148 KiB
assert channel_strike_boot_lds(CHANNEL_STRIKE_BOOT_LDS_TERMS // 16, 1, BOOT_MAX_REPLICATES, True) \
    + CHANNEL_STRIKE_BOOT_LDS_STATIC == 148 * 1024 + 288 <= LDS_BYTES


class sc_lateral_fit(C.Structure):
    """One row of sc_lateral_offsets / sc_lateral_offsets_dem (docs/lateral.md)."""
    _fields_ = [("cell", C.c_int64), ("n", C.c_int32), ("lag", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32),
                ("status", C.c_int32),
                ("offset", C.c_double), ("offset_lo", C.c_double), ("offset_hi", C.c_double),
                ("mse", C.c_double), ("rho", C.c_double), ("dz", C.c_double), ("tilt", C.c_double)]


LATERAL_FIT_DTYPE = np.dtype(sc_lateral_fit)
LATERAL_MAX_LAG, LATERAL_MAX_BAND, LATERAL_MAX_FAR = 255, 64, 1024     # SC_LATERAL_MAX_*


class sc_surface_row(C.Structure):
    """One row of sc_snr_surface (docs/surface.md)."""
    _fields_ = [("par_index", C.c_int32), ("ang_index", C.c_int32), ("par_lo", C.c_int32), ("par_hi", C.c_int32),
                ("ang_lo", C.c_int32), ("ang_hi", C.c_int32), ("n_within", C.c_int32), ("status", C.c_int32),
                ("snr", C.c_double), ("amp", C.c_double)]


SURFACE_ROW_DTYPE = np.dtype(sc_surface_row)
SURFACE_MAX_TEMPLATES = 65535                                          # (sc_snr_surface refuses more)
SURFACE_CELL_BATCH = 8                                                 # SF_CB of sc_surface.hip: cells per workgroup of k_sf_score


class sc_xfer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("kind", C.c_int32),
                ("sy0", C.c_int32), ("sx0", C.c_int32),
                ("dy0", C.c_int32), ("dx0", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32)]


_P = C.c_void_p
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint32)
_bp = C.POINTER(C.c_uint8)
_llp = C.POINTER(C.c_longlong)
_ip = C.POINTER(C.c_int32)
_i, _d, _ll, _v = C.c_int, C.c_double, C.c_longlong, C.c_void_p

# the pieces the fit family's prototypes are made of (include/scarplet_hip.h), in the order they stand in one
_DEM = [_dp, _i, _i]                      # z, ny, nx: the prefix of every _dem form
_CELLS = [_llp, _dp, _dp, _ll]            # cells, sa, ca, K
_SEGS = [_llp, _ip, _ll]                  # seg_start, seg_label, S
_AGES = [_dp, _i]                         # ages, A
_HW = [_i, _i]                            # h, w
_STOP = [_d, _d, _i]                      # de, delta, min_samples
_ROBUST = [_dp, _i, _d, _i, _d]           # weights, loss, tuning, iterations, scale
_RAMP = [_i, _i, _d]                      # width, mode, slope
_CELL_OUT = [_v, _dp]                     # rows, curves
_SEG_OUT = [_v, _v, _dp]                  # rows, cell table, curves


def _fit_pair(name, *pieces):
    """The table entries of a fit call and of its _dem twin, from one description: the context, (z, ny, nx) for the
    twin, then ``pieces`` in order."""
    own = [t for p in pieces for t in p]
    return {name: (_i, [_P] + own), name + "_dem": (_i, [_P] + _DEM + own)}


# every symbol include/scarplet_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "sc_abi_version": (C.c_int, []),
    "sc_build_id": (C.c_char_p, []),
    "sc_device_count": (C.c_int, []),
    "sc_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "sc_destroy": (None, [_P]),
    "sc_last_error": (C.c_char_p, [_P]),
    "sc_set_dem": (C.c_int, [_P, _dp] + [C.c_int] * 10 + [C.c_double] * 2
                   + [C.c_int, _dp, _dp]),
    "sc_dem_info": (C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]),
    "sc_set_dem_device": (C.c_int, [_P, _P] + [C.c_int] * 10
                          + [C.c_double] * 2 + [C.c_int, _dp, _dp]),
    "sc_upload_window": (C.c_int, [_P, _dp, C.c_int, C.c_int,
                                   C.POINTER(C.c_int)]),
    "sc_set_masks": (C.c_int, [_P, C.c_int, _bp, _bp]),
    "sc_clear_windows": (C.c_int, [_P]),
    "sc_crater_windows": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int), _dp, _dp, _dp]),
    "sc_reset_best": (C.c_int, [_P]),
    "sc_match": (C.c_int, [_P, C.POINTER(sc_template), C.c_int,
                           C.POINTER(sc_plan)]),
    "sc_match_async": (C.c_int, [_P, C.POINTER(sc_template), C.c_int,
                                 C.POINTER(sc_plan)]),
    "sc_sync": (C.c_int, [_P]),
    "sc_match_template": (C.c_int, [_P, C.POINTER(sc_template),
                                    C.POINTER(sc_plan), _fp, _fp]),
    "sc_get_best": (C.c_int, [_P, _fp, _fp, _up]),
    "sc_get_result": (C.c_int, [_P, _dp, _dp, C.c_int, _dp]),
    "sc_compare_begin": (C.c_int, [_P, C.c_int, C.c_int]),
    "sc_compare_fold": (C.c_int, [_P, _dp, _dp, C.c_double, C.c_double]),
    "sc_compare_fold_planes": (C.c_int, [_P, _dp, _dp, _dp, _dp]),
    "sc_compare_end": (C.c_int, [_P, _dp, _dp, _dp, _dp]),
    "sc_set_option": (C.c_int, [_P, C.c_char_p, C.c_double]),
    "sc_forget_templates": (C.c_int, [_P]),
    "sc_templ_cache_info": (C.c_int, [_P] + [C.POINTER(C.c_longlong)] * 5),
    "sc_fill_nodata": (C.c_int, [_P, _dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                 C.POINTER(C.c_longlong)]),
    "sc_curvature": (C.c_int, [_P, C.c_double, C.c_double, C.c_double, _fp]),
    "sc_curvature_f64": (C.c_int, [_P] + [C.c_double] * 4 + [_dp]),
    "sc_curvature_noise": (C.c_int, [_P, _dp, C.c_int, _bp, _dp]),
    "sc_get_near_ties": (C.c_int, [_P, _bp]),
    "sc_score_cells_f64": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.c_int, _dp, _dp]),
    "sc_get_near_events": (C.c_int, [_P, _up, C.c_longlong, C.POINTER(C.c_longlong)]),
    "sc_score_pairs_f64": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, _dp, _dp]),
    "sc_settle_exact": (C.c_int, [_P, C.c_int, C.c_double, C.POINTER(C.c_longlong)]),
    "sc_snapshot_best": (C.c_int, [_P]),
    "sc_set_best": (C.c_int, [_P, _fp, _fp, _up]),
    "sc_rank_candidates": (C.c_int, [_P, _up, C.c_longlong, C.POINTER(C.c_longlong)]),
    "sc_settle_pairs": (C.c_int, [_P, C.POINTER(sc_template), C.c_int, _up, C.c_longlong, C.c_int, C.c_double,
                                  C.POINTER(C.c_longlong)]),
    "sc_exchange_candidates": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "sc_trace_planes": (C.c_int, [_P, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_longlong, _bp,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_longlong)]),
    "sc_trace_result": (C.c_int, [_P, _dp, _dp, C.c_int, C.c_double, C.c_double, C.c_longlong, _bp,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_longlong)]),
    "sc_trace_segments": (C.c_int, [_P, C.c_void_p, C.c_longlong]),
    # the fit family: each call and its _dem twin from one line.  Between (h, w) and de stands what the call fits besides
    # the age - D, the refinement depth, or (width, mode, slope); the robust block follows min_samples / min_profiles; an
    # int8 plane comes last
    **_fit_pair("sc_fit_profiles", _CELLS, _AGES, _HW, _STOP, _CELL_OUT),
    **_fit_pair("sc_fit_profiles_robust", _CELLS, _AGES, _HW, _STOP, _ROBUST, _CELL_OUT),
    **_fit_pair("sc_fit_profiles_ramp", _CELLS, _AGES, _HW, _RAMP, _STOP, _CELL_OUT, [_v]),
    **_fit_pair("sc_fit_profiles_refine", _CELLS, _AGES, _HW, [_i], _STOP, _CELL_OUT),
    **_fit_pair("sc_fit_segments", _CELLS, _SEGS, _AGES, _HW, _STOP, [_i], _SEG_OUT),
    **_fit_pair("sc_fit_profiles_shift", _CELLS, _AGES, _HW, [_i], _STOP, _CELL_OUT, [_v]),
    **_fit_pair("sc_fit_segments_shift", _CELLS, _SEGS, _AGES, _HW, [_i], _STOP, [_i], _SEG_OUT, [_v]),
    **_fit_pair("sc_fit_segments_ramp", _CELLS, _SEGS, _AGES, _HW, _RAMP, _STOP, [_i], _SEG_OUT, [_v]),
    **_fit_pair("sc_fit_segments_robust", _CELLS, _SEGS, _AGES, _HW, _STOP, [_i], _ROBUST, _SEG_OUT),
    **_fit_pair("sc_fit_segments_refine", _CELLS, _SEGS, _AGES, _HW, [_i], _STOP, [_i], _SEG_OUT),
    # (seg_blk_start, blk_start, NB; then D, de, min_samples, min_profiles, min_blocks, R, level, seed; rows, hist, idx, amp)
    **_fit_pair("sc_bootstrap_segments", _CELLS, _SEGS, [_llp, _llp, _ll], _AGES, _HW, [_i, _d, _i, _i, _i, _i, _d, C.c_uint64],
                [_v, _v, _v, _dp]),
    # (seg_win_start, win_lo, win_hi, NW; then D, de, delta, min_samples, min_profiles)
    **_fit_pair("sc_fit_strike", _CELLS, _SEGS, [_llp, _llp, _llp, _ll], _AGES, _HW, [_i], _STOP, [_i], _CELL_OUT),
    # (the windows as sc_fit_strike; D, de, min_samples, min_profiles; win_blk_start, blk_hi, NWB; min_blocks, R, level, seed;
    # rows, hist)
    **_fit_pair("sc_strike_bootstrap", _CELLS, _SEGS, [_llp, _llp, _llp, _ll], _AGES, _HW, [_i, _d, _i, _i], [_llp, _llp, _ll],
                [_i, _i, _d, C.c_uint64], [_v, _v]),
    # (h, q0, q1, D: no age grid)
    **_fit_pair("sc_lateral_offsets", _CELLS, [_i, _i, _i, _i], _STOP, _CELL_OUT),
    # (sc_fit_profiles_shift's list, the frequencies and F for the ages and A)
    **_fit_pair("sc_channel_profiles", _CELLS, _AGES, _HW, [_i], _STOP, _CELL_OUT, [_v]),
    # (sc_fit_segments_shift's list with the depth mode behind D)
    **_fit_pair("sc_channel_segments", _CELLS, _SEGS, _AGES, _HW, [_i, _i], _STOP, [_i], _SEG_OUT, [_v]),
    # (sc_bootstrap_segments' list with the depth mode behind D)
    **_fit_pair("sc_channel_bootstrap", _CELLS, _SEGS, [_llp, _llp, _ll], _AGES, _HW,
                [_i, _i, _d, _i, _i, _i, _i, _d, C.c_uint64], [_v, _v, _v, _dp]),
    # (sc_fit_strike's list with the depth mode behind D; the sums of the shifts come last)
    **_fit_pair("sc_channel_strike", _CELLS, _SEGS, [_llp, _llp, _llp, _ll], _AGES, _HW, [_i, _i], _STOP, [_i], _CELL_OUT, [_v]),
    # (sc_strike_bootstrap's list with the depth mode behind D)
    **_fit_pair("sc_channel_strike_bootstrap", _CELLS, _SEGS, [_llp, _llp, _llp, _ll], _AGES, _HW, [_i, _i, _d, _i, _i],
                [_llp, _llp, _ll], [_i, _i, _d, C.c_uint64], [_v, _v]),
    "sc_snr_surface": (C.c_int, [_P, C.POINTER(sc_template), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_longlong, C.c_double,
                                 C.c_void_p, _dp, _dp]),
    "sc_get_resolution_stats": (C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "sc_get_template_sums": (C.c_int, [_P, C.c_int, _dp, _dp]),
    "sc_profile": (C.c_int, [_P, C.c_int]),
    "sc_profile_get": (C.c_int, [_P, C.c_int, C.POINTER(C.c_longlong), _dp]),
    "sc_kernel_name": (C.c_char_p, [C.c_int]),
    "sc_device_bytes": (C.c_size_t, [_P]),
    "sc_comm_unique_id": (C.c_int, [_P]),
    "sc_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "sc_gather_result": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                   _dp, _dp, C.c_int, _dp]),
    "sc_halo_exchange": (C.c_int, [_P, _dp] + [C.c_int] * 6
                         + [C.POINTER(sc_xfer), C.c_int, C.POINTER(_P)]),
    "sc_fold_ranks": (C.c_int, [_P]),
    "sc_comm_destroy": (C.c_int, [_P]),
    "sc_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                               C.c_char_p, C.c_int]),
}

_lib = None


def load():
    """Load the shared library (once) and bind every exported function."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScarpletHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as "
            "g; g.build()'` or `make -C scarplet_amd/csrc` (needs hipcc); this "
            "package has no CPU fallback" % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise ScarpletHipError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = ABI mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.sc_abi_version() != ABI_VERSION:
        raise ScarpletHipError("libscarplet_hip.so ABI %d != expected %d"
                               % (lib.sc_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _as(arr, ptr_type):
    return arr.ctypes.data_as(ptr_type)


def _arg(a, t):
    """``a`` as an argument of type ``t``: an array as that pointer, None (an output not asked for) as it is, a number
    as a float where ``t`` is a double and as an int elsewhere."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(t)
    return float(a) if t is C.c_double else int(a)


SPECTRA_MB = 8192.0
TEMPL_GB_AUTO = -1.0        # option "templ_gb": the automatic budget (half of the free device memory); 0 is off


class Context(object):
    """One GPU's matcher state (an ``sc_ctx``)."""

    def __init__(self, device=0):
        self.lib = load()
        n = self.lib.sc_device_count()
        if n <= 0:
            raise ScarpletHipError(
                "no HIP device visible: scarplet_amd needs an AMD GPU "
                "(MI355X / gfx950); there is no CPU fallback")
        self._h = _P()
        rc = self.lib.sc_create(int(device), C.byref(self._h))
        if rc != SC_OK:
            raise ScarpletHipError("sc_create(device=%d) failed: %d"
                                   % (device, rc))
        self.device = int(device)
        self.core = None
        self.dem_key = None        # (geometry, cell size, the device's 128-bit fingerprint) of the resident block
        self.dem_nan = 0           # NaN cells the device found in it
        self.dem_unchanged = False # the last set_dem handed over what the context already held
        self.spectra_mb = 0.0
        self.variant = 0           # option "variant" as last set (0: none)
        self.masked_slots = set()  # window slots whose templates carry per-cell masks (set_masks)
        # searches small enough for it keep their curvature spectra (sc_set_option "spectra_mb"): the
        # next search of the same DEM with the same tiles and orientations - the next scale of a
        # multi-scale job - starts from them
        self.set_option("spectra_mb", SPECTRA_MB)

    # -- plumbing ----------------------------------------------------------
    def _check(self, rc, what):
        if rc != SC_OK:
            msg = self.lib.sc_last_error(self._h)
            raise ScarpletHipError("%s failed (%d): %s" % (
                what, rc, msg.decode() if msg else ""))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.sc_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """Engine options (include/scarplet_hip.h sc_set_option): 'kappa',
        'variant', 'y_gb', 'spectra_mb', 'templ_gb', 'fuse_fwd', 'fit_chunk', 'channel_terms'."""
        self._check(self.lib.sc_set_option(self._h, name.encode(), float(value)),
                    "sc_set_option(%s)" % name)
        if name == "spectra_mb":
            self.spectra_mb = float(value)
        elif name == "variant":
            self.variant = int(value)   # (Matcher.can_flag_near_ties: variant 9 turns the fast row kernel off)

    def forget_spectra(self):
        """Drop the curvature spectra kept from earlier searches (option
        'spectra_mb'): the next search computes its own again."""
        self.set_option("spectra_mb", self.spectra_mb)

    def forget_templates(self):
        """Drop the template coefficient planes kept across searches (option 'templ_gb'): the next
        search runs the templates' forward chain again."""
        self._check(self.lib.sc_forget_templates(self._h), "sc_forget_templates")

    def templ_cache_info(self):
        """The template cache since the context was made: ``hits`` / ``misses`` in orientation
        runs, ``entries`` and ``bytes`` held now, ``evictions``."""
        v = [C.c_longlong(0) for _ in range(5)]
        self._check(self.lib.sc_templ_cache_info(self._h, *[C.byref(x) for x in v]), "sc_templ_cache_info")
        return dict(zip(("hits", "misses", "entries", "bytes", "evictions"), (int(x.value) for x in v)))

    def fill_nodata(self, z, max_search_distance, smoothing_iterations=0):
        """One GDALFillNodata-style pass over ``z`` (float64, NaN = nodata), in
        place; returns the number of cells still nodata."""
        assert z.dtype == np.float64 and z.flags.c_contiguous and z.ndim == 2
        left = C.c_longlong(0)
        self._check(self.lib.sc_fill_nodata(self._h, _as(z, _dp), z.shape[0], z.shape[1],
                                            float(max_search_distance), int(smoothing_iterations),
                                            C.byref(left)), "sc_fill_nodata")
        return int(left.value)

    # -- DEM ----------------------------------------------------------------
    def _dem_args(self, ly, lx, origin, shape, core, wrap):
        ny, nx = shape
        gy0, gx0 = origin
        if core is None:
            core = (0, ny, 0, nx)
        self.core = tuple(int(v) for v in core)
        self.shape = (int(ny), int(nx))
        return [int(ly), int(lx), int(gy0), int(gx0), int(ny), int(nx)] \
            + list(self.core)

    def set_dem(self, z, dx, dy, xaxis, yaxis, origin=(0, 0), shape=None,
                core=None, wrap=True):
        z = np.ascontiguousarray(z, dtype=np.float64)
        ly, lx = z.shape
        shape = z.shape if shape is None else shape
        xa = np.ascontiguousarray(xaxis, dtype=np.float64)
        ya = np.ascontiguousarray(yaxis, dtype=np.float64)
        assert xa.size == shape[1] and ya.size == shape[0]
        args = self._dem_args(ly, lx, origin, shape, core, wrap)
        self.dem_key = None
        self._check(self.lib.sc_set_dem(
            self._h, _as(z, _dp), *args, float(dx), float(dy), int(bool(wrap)),
            _as(xa, _dp), _as(ya, _dp)), "sc_set_dem")
        self._dem_info(args, dx, dy, wrap)

    def _dem_info(self, args, dx, dy, wrap):
        """What the device found in the block just handed over (sc_dem_info): NaN cells, the
        fingerprint, and whether it is the block the context already held."""
        nan, h2, same = C.c_longlong(0), (C.c_ulonglong * 2)(), C.c_int(0)
        self._check(self.lib.sc_dem_info(self._h, C.byref(nan), h2, C.byref(same)), "sc_dem_info")
        self.dem_nan, self.dem_unchanged = int(nan.value), bool(same.value)
        self.dem_key = (tuple(args), float(dx), float(dy), bool(wrap), int(h2[0]), int(h2[1]))

    def set_dem_device(self, z_dev, ly, lx, dx, dy, xaxis, yaxis, origin,
                       shape, core):
        xa = np.ascontiguousarray(xaxis, dtype=np.float64)
        ya = np.ascontiguousarray(yaxis, dtype=np.float64)
        args = self._dem_args(ly, lx, origin, shape, core, False)
        self.dem_key = None
        self._check(self.lib.sc_set_dem_device(
            self._h, z_dev, *args, float(dx), float(dy), 0, _as(xa, _dp),
            _as(ya, _dp)), "sc_set_dem_device")
        self._dem_info(args, dx, dy, False)

    def core_shape(self):
        cy0, cy1, cx0, cx1 = self.core
        return cy1 - cy0, cx1 - cx0

    def curvature(self, cc, sc2, ss, block_shape):
        out = np.empty(block_shape, dtype=np.float32)
        self._check(self.lib.sc_curvature(self._h, cc, sc2, ss, _as(out, _fp)),
                    "sc_curvature")
        return out

    def curvature_f64(self, alpha, block_shape):
        """dem.py:68-107 in float64 (sc_curvature_f64); cos / sin / squares by numpy, as the
        reference evaluates them."""
        out = np.empty(block_shape, dtype=np.float64)
        self._check(self.lib.sc_curvature_f64(self._h, float(np.cos(alpha) ** 2), float(np.sin(alpha)),
                                              float(np.cos(alpha)), float(np.sin(alpha) ** 2),
                                              _as(out, _dp)), "sc_curvature_f64")
        return out

    def curvature_noise(self, weights, nan_mask=None):
        """sc_curvature_noise: (n, mean[3], C[6]) of the high-passed stencil planes over all cells, then over
        the cells farther than the filter radius from every cell ``nan_mask`` flags (20 float64)."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert w.ndim == 1 and w.size % 2 == 1
        m = None
        if nan_mask is not None:
            m = np.ascontiguousarray(nan_mask, dtype=np.uint8)
            assert m.shape == self.shape
        out = np.empty(20, dtype=np.float64)
        self._check(self.lib.sc_curvature_noise(self._h, _as(w, _dp), w.size // 2,
                                                None if m is None else _as(m, _bp), _as(out, _dp)),
                    "sc_curvature_noise")
        return out

    # -- generic plugin windows --------------------------------------------
    def upload_window(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        slot = C.c_int(-1)
        self._check(self.lib.sc_upload_window(
            self._h, _as(w, _dp), w.shape[0], w.shape[1], C.byref(slot)),
            "sc_upload_window")
        return slot.value

    def set_masks(self, slot, limits=None, err=None):
        def conv(m):
            if m is None:
                return None, None
            a = np.ascontiguousarray(m, dtype=np.uint8)
            return a, _as(a, _bp)
        la, lp = conv(limits)
        ea, ep = conv(err)
        self._check(self.lib.sc_set_masks(self._h, slot, lp, ep),
                    "sc_set_masks")
        # (the slots whose templates carry per-cell masks: Matcher.can_flag_near_ties)
        if lp is not None or ep is not None:
            self.masked_slots.add(int(slot))
        else:
            self.masked_slots.discard(int(slot))

    def clear_windows(self):
        self._check(self.lib.sc_clear_windows(self._h), "sc_clear_windows")
        self.masked_slots.clear()

    def crater_windows(self, tables, return_windows=False):
        """sc_crater_windows for the tables of ``WindowedTemplate.crater_tables``: the Crater windows of every (radius,
        age), radius-major, synthesised into window slots.  Returns (slots, count(W != 0), sum(W * W)) - and, with
        ``return_windows``, the list of float64 windows as the device made them.  A support box that leaves the grid
        is a ValueError."""
        n_r, n_a = len(tables["boxes"]), len(tables["age_tab"])
        arrs = {k: np.ascontiguousarray(tables[k], dtype=np.float64) for k in ("theta_tab", "dxy", "ring", "age_tab")}
        n_th = len(arrs["theta_tab"])
        assert arrs["theta_tab"].shape == (n_th, 3) and arrs["dxy"].shape == (n_r, n_th, 2) \
            and arrs["ring"].shape == (n_r, 2) and arrs["age_tab"].shape == (n_a, 2)
        boxes = np.ascontiguousarray(tables["boxes"], dtype=np.int32)
        assert boxes.shape == (n_r, 4)
        slots = np.empty(n_r * n_a, dtype=np.intc)
        count, sumsq = np.empty(n_r * n_a), np.empty(n_r * n_a)
        sizes = np.repeat((boxes[:, 1] - boxes[:, 0] + 1).astype(np.int64) * (boxes[:, 3] - boxes[:, 2] + 1), n_a)
        w = np.empty(int(sizes.sum()) if return_windows and (sizes > 0).all() else 0)
        rc = self.lib.sc_crater_windows(self._h, n_r, n_a, n_th, _as(arrs["theta_tab"], _dp), _as(arrs["dxy"], _dp),
                                        _as(arrs["ring"], _dp), _as(arrs["age_tab"], _dp), float(tables["d_half"]),
                                        boxes.ctypes.data_as(C.POINTER(C.c_int32)), slots.ctypes.data_as(C.POINTER(C.c_int)),
                                        _as(count, _dp), _as(sumsq, _dp), _as(w, _dp) if w.size else None)
        if rc == SC_ERR_INVALID:
            msg = self.lib.sc_last_error(self._h)
            raise ValueError(msg.decode() if msg else "sc_crater_windows: bad argument")
        self._check(rc, "sc_crater_windows")
        if not return_windows:
            return slots, count, sumsq
        ends = np.cumsum(sizes)
        shapes = np.repeat(np.stack([boxes[:, 1] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 2] + 1], 1), n_a, axis=0)
        wins = [w[e - n:e].reshape(sh) for e, n, sh in zip(ends, sizes, shapes)]
        return slots, count, sumsq, wins

    # -- hot path -----------------------------------------------------------
    def reset_best(self):
        self._check(self.lib.sc_reset_best(self._h), "sc_reset_best")

    def match(self, templates, plan, sync=True):
        fn = self.lib.sc_match if sync else self.lib.sc_match_async
        self._check(fn(self._h, templates, len(templates), C.byref(plan)),
                    "sc_match")

    def sync(self):
        self._check(self.lib.sc_sync(self._h), "sc_sync")

    def match_template(self, template, plan):
        h, w = self.core_shape()
        amp = np.empty((h, w), dtype=np.float32)
        snr = np.empty((h, w), dtype=np.float32)
        self._check(self.lib.sc_match_template(
            self._h, C.byref(template), C.byref(plan), _as(amp, _fp),
            _as(snr, _fp)), "sc_match_template")
        return amp, snr

    def get_best(self):
        h, w = self.core_shape()
        amp = np.empty((h, w), dtype=np.float32)
        snr = np.empty((h, w), dtype=np.float32)
        idx = np.empty((h, w), dtype=np.uint32)
        self._check(self.lib.sc_get_best(self._h, _as(amp, _fp), _as(snr, _fp),
                                         _as(idx, _up)), "sc_get_best")
        return amp, snr, idx

    def get_result(self, param_of_id, angle_of_id):
        """(4, h, w) float64: amp, age, angle, snr of the running best."""
        h, w = self.core_shape()
        par = np.ascontiguousarray(param_of_id, dtype=np.float64)
        ang = np.ascontiguousarray(angle_of_id, dtype=np.float64)
        # (large results are views of recycled host blocks, already faulted in: _hostpool)
        from scarplet_amd import _hostpool
        out = _hostpool.empty((4, h, w), dtype=np.float64)
        self._check(self.lib.sc_get_result(self._h, _as(par, _dp), _as(ang, _dp),
                                           len(par), _as(out, _dp)), "sc_get_result")
        return out

    def template_sums(self, n):
        a = np.empty(n)
        b = np.empty(n)
        self._check(self.lib.sc_get_template_sums(self._h, n, _as(a, _dp),
                                                  _as(b, _dp)),
                    "sc_get_template_sums")
        return a, b

    # -- traces of a result (docs/traces.md) ---------------------------------------
    def _trace_out(self, shape, rc_fn, what):
        thin = np.empty(shape, dtype=np.uint8)
        labels = np.empty(shape, dtype=np.int32)
        k = C.c_longlong(0)
        self._check(rc_fn(_as(thin, _bp), labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)), what)
        seg = np.empty(int(k.value), dtype=SEGMENT_DTYPE)
        if k.value:
            self._check(self.lib.sc_trace_segments(self._h, seg.ctypes.data_as(C.c_void_p), k.value), "sc_trace_segments")
        return thin, labels, seg

    def trace_planes(self, planes, snr_low, snr_high, min_cells):
        """sc_trace_planes on a (4, ny, nx) float64 C-contiguous host array: (thin u8, labels int32, table)."""
        assert planes.dtype == np.float64 and planes.flags.c_contiguous and planes.ndim == 3 and planes.shape[0] == 4
        ny, nx = planes.shape[1:]
        return self._trace_out((ny, nx), lambda t, l, k: self.lib.sc_trace_planes(
            self._h, _as(planes, _dp), ny, nx, float(snr_low), float(snr_high), int(min_cells), t, l, k),
            "sc_trace_planes")

    def trace_result(self, param_of_id, angle_of_id, snr_low, snr_high, min_cells):
        """sc_trace_result: the same on the planes get_result would return, formed and traced on the device."""
        par = np.ascontiguousarray(param_of_id, dtype=np.float64)
        ang = np.ascontiguousarray(angle_of_id, dtype=np.float64)
        return self._trace_out(self.core_shape(), lambda t, l, k: self.lib.sc_trace_result(
            self._h, _as(par, _dp), _as(ang, _dp), len(par), float(snr_low), float(snr_high), int(min_cells), t, l, k),
            "sc_trace_result")

    # -- the fit family: one frame, then what each call has of its own -------------------
    def _fit_call(self, name, z, cells, segs, ages, own):
        """One call of the fit family: ``name`` on the context's DEM, or its _dem twin on ``z`` (float64, C-contiguous, 2-D).
        ``cells``: (cells, sa, ca), int64 and float64; ``segs``: None, or (seg_start, seg_label) int64 and int32, then the
        int64 arrays that follow them in the prototype and their count; ``ages``: None or the float64 grid; ``own``: the
        call's scalars and outputs in the prototype's order.  Every array is 1-D and C-contiguous, the heads of one length;
        every argument goes over as the type SIGNATURES has at its position (``_arg``)."""
        idx, sa, ca = cells
        K = len(idx)
        assert len(sa) == K and len(ca) == K
        arrays = [(idx, np.int64), (sa, np.float64), (ca, np.float64)]
        args = [idx, sa, ca, K]
        if segs is not None:
            seg_start, seg_label = segs[:2]
            assert len(seg_start) == len(seg_label) + 1
            arrays += [(seg_start, np.int64), (seg_label, np.int32)] + [(a, np.int64) for a in segs[2:-1]]
            args += [seg_start, seg_label, len(seg_label)] + list(segs[2:])
        if ages is not None:
            arrays.append((ages, np.float64))
            args += [ages, len(ages)]
        for a, t in arrays:
            assert a.dtype == t and a.ndim == 1 and a.flags.c_contiguous
        args += own
        if z is not None:
            assert z.dtype == np.float64 and z.ndim == 2 and z.flags.c_contiguous
            name += "_dem"
            args = [z, z.shape[0], z.shape[1]] + args
        types = SIGNATURES[name][1][1:]
        assert len(args) == len(types)
        self._check(getattr(self.lib, name)(self._h, *[_arg(a, t) for a, t in zip(args, types)]), name)

    # -- scarp-profile dating (docs/profiles.md) ------------------------------------
    def fit_profiles(self, cells, sa, ca, ages, h, w, de, delta, min_samples, curve=False, z=None, shift=None,
                     shift_plane=False):
        """sc_fit_profiles on the context's DEM, or sc_fit_profiles_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, curve or None).  cells int64, sa / ca / ages float64, all 1-D and C-contiguous.  With ``shift`` (D, the
        range of the centre shift in cells) the _shift calls: (rows, curve or None, (K, A) int8 shifts or None)."""
        K, A = len(cells), len(ages)
        rows = np.zeros(K, dtype=PROFILE_DTYPE if shift is None else PROFILE_SHIFT_DTYPE)
        sse = np.empty((K, A), dtype=np.float64) if curve else None
        if shift is None:
            self._fit_call("sc_fit_profiles", z, (cells, sa, ca), None, ages, [h, w, de, delta, min_samples, rows, sse])
            return rows, sse
        plane = np.zeros((K, A), dtype=np.int8) if shift_plane else None
        self._fit_call("sc_fit_profiles_shift", z, (cells, sa, ca), None, ages,
                       [h, w, shift, de, delta, min_samples, rows, sse, plane])
        return rows, sse, plane

    def channel_profiles(self, cells, sa, ca, frequencies, h, w, D, de, delta, min_samples, curve=False, shift_plane=False,
                         z=None):
        """sc_channel_profiles on the context's DEM, or sc_channel_profiles_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, (K, F) float64 sse* curves or None, (K, F) int8 shifts or None).  cells int64, sa / ca / frequencies float64,
        all 1-D and C-contiguous; ``D``: the range of the centre shift in cells.  The rows are sc_profile_shift_fit, kt
        carrying f (docs/channels.md)."""
        K, F = len(cells), len(frequencies)
        rows = np.zeros(K, dtype=PROFILE_SHIFT_DTYPE)
        sse = np.empty((K, F), dtype=np.float64) if curve else None
        plane = np.zeros((K, F), dtype=np.int8) if shift_plane else None
        self._fit_call("sc_channel_profiles", z, (cells, sa, ca), None, frequencies,
                       [h, w, D, de, delta, min_samples, rows, sse, plane])
        return rows, sse, plane

    def channel_segments(self, cells, sa, ca, seg_start, seg_label, frequencies, h, w, D, mode, de, delta, min_samples,
                         min_profiles, cell_table=False, curve=False, shift_plane=False, z=None):
        """sc_channel_segments on the context's DEM, or sc_channel_segments_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, cell table or None, (S, F) float64 pooled curves or None, (K, F) int8 shifts or None).  The arrays as
        fit_segments takes them, the cells grouped by reach; ``D``: the range of the centre shift in cells; ``mode``:
        CHANNEL_DEPTH_PROFILE or CHANNEL_DEPTH_SEGMENT.  The rows are sc_segment_fit, kt carrying f (docs/channels.md)."""
        K, F, S = len(cells), len(frequencies), len(seg_label)
        rows = np.zeros(S, dtype=SEGMENT_FIT_DTYPE)
        tab = np.zeros(K, dtype=CHANNEL_SEGMENT_CELL_DTYPE) if cell_table else None
        sse = np.empty((S, F), dtype=np.float64) if curve else None
        plane = np.zeros((K, F), dtype=np.int8) if shift_plane else None
        self._fit_call("sc_channel_segments", z, (cells, sa, ca), (seg_start, seg_label), frequencies,
                       [h, w, D, mode, de, delta, min_samples, min_profiles, rows, tab, sse, plane])
        return rows, tab, sse, plane

    @staticmethod
    def _check_weights(weights, z):
        """``weights``: None or a float64, C-contiguous plane of the DEM's shape (the caller's check where z is the
        context's)."""
        if weights is not None:
            assert weights.dtype == np.float64 and weights.ndim == 2 and weights.flags.c_contiguous
            assert z is None or weights.shape == z.shape

    def fit_profiles_robust(self, cells, sa, ca, ages, h, w, de, delta, min_samples, weights=None, loss=ROBUST_NONE,
                            tuning=0.0, iterations=1, scale=0.0, curve=False, z=None):
        """sc_fit_profiles_robust on the context's DEM, or sc_fit_profiles_robust_dem on ``z`` (float64, C-contiguous,
        2-D): (rows, (K, A) float64 loss curves or None).  cells int64, sa / ca / ages float64, all 1-D and C-contiguous;
        ``weights``: None or a float64, C-contiguous plane of the DEM's shape; ``scale`` 0: estimated per profile."""
        self._check_weights(weights, z)
        K, A = len(cells), len(ages)
        rows = np.zeros(K, dtype=PROFILE_ROBUST_DTYPE)
        out = np.empty((K, A), dtype=np.float64) if curve else None
        self._fit_call("sc_fit_profiles_robust", z, (cells, sa, ca), None, ages,
                       [h, w, de, delta, min_samples, weights, loss, tuning, iterations, scale, rows, out])
        return rows, out

    def fit_profiles_ramp(self, cells, sa, ca, ages, h, w, de, delta, min_samples, width, mode=RAMP_FREE, slope=0.0,
                          curve=False, width_plane=False, z=None):
        """sc_fit_profiles_ramp on the context's DEM, or sc_fit_profiles_ramp_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, curve or None, (K, A) int8 half-widths or None).  cells int64, sa / ca / ages float64, all 1-D and
        C-contiguous; ``width``: M, the range of the half-width in cells; ``slope`` is read with RAMP_SLOPE alone."""
        K, A = len(cells), len(ages)
        rows = np.zeros(K, dtype=PROFILE_RAMP_DTYPE)
        sse = np.empty((K, A), dtype=np.float64) if curve else None
        plane = np.zeros((K, A), dtype=np.int8) if width_plane else None
        self._fit_call("sc_fit_profiles_ramp", z, (cells, sa, ca), None, ages,
                       [h, w, width, mode, slope, de, delta, min_samples, rows, sse, plane])
        return rows, sse, plane

    def fit_profiles_refine(self, cells, sa, ca, ages, h, w, de, delta, min_samples, refine, curve=False, z=None):
        """sc_fit_profiles_refine on the context's DEM, or sc_fit_profiles_refine_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, curve or None).  cells int64, sa / ca / ages float64, all 1-D and C-contiguous; ``refine``: R, the levels of
        64 candidate ages below the grid."""
        K, A = len(cells), len(ages)
        rows = np.zeros(K, dtype=PROFILE_FINE_DTYPE)
        sse = np.empty((K, A), dtype=np.float64) if curve else None
        self._fit_call("sc_fit_profiles_refine", z, (cells, sa, ca), None, ages,
                       [h, w, refine, de, delta, min_samples, rows, sse])
        return rows, sse

    # -- one age per trace segment (docs/segments.md) -------------------------------
    def fit_segments(self, cells, sa, ca, seg_start, seg_label, ages, h, w, de, delta, min_samples, min_profiles,
                     cell_table=False, curve=False, z=None, shift=None, shift_plane=False):
        """sc_fit_segments on the context's DEM, or sc_fit_segments_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, cell table or None, curve or None).  cells and seg_start int64, seg_label int32, sa / ca / ages
        float64, all 1-D and C-contiguous; the cells grouped by segment.  With ``shift`` (D, the range of the centre
        shift in cells) the _shift calls: (rows, cell table or None, curve or None, (K, A) int8 shifts or None)."""
        K, A, S = len(cells), len(ages), len(seg_label)
        rows = np.zeros(S, dtype=SEGMENT_FIT_DTYPE)
        tab = np.zeros(K, dtype=SEGMENT_CELL_DTYPE if shift is None else SEGMENT_SHIFT_CELL_DTYPE) if cell_table else None
        sse = np.empty((S, A), dtype=np.float64) if curve else None
        if shift is None:
            self._fit_call("sc_fit_segments", z, (cells, sa, ca), (seg_start, seg_label), ages,
                           [h, w, de, delta, min_samples, min_profiles, rows, tab, sse])
            return rows, tab, sse
        plane = np.zeros((K, A), dtype=np.int8) if shift_plane else None
        self._fit_call("sc_fit_segments_shift", z, (cells, sa, ca), (seg_start, seg_label), ages,
                       [h, w, shift, de, delta, min_samples, min_profiles, rows, tab, sse, plane])
        return rows, tab, sse, plane

    def fit_segments_ramp(self, cells, sa, ca, seg_start, seg_label, ages, h, w, de, delta, min_samples, min_profiles, width,
                          mode=RAMP_FREE, slope=0.0, cell_table=False, curve=False, width_plane=False, z=None):
        """sc_fit_segments_ramp on the context's DEM, or sc_fit_segments_ramp_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, cell table or None, curve or None, (S, A) int8 half-widths or None).  The arrays as fit_segments takes
        them; ``width``: M, the range of the half-width in cells; ``slope`` is read with RAMP_SLOPE alone."""
        K, A, S = len(cells), len(ages), len(seg_label)
        rows = np.zeros(S, dtype=SEGMENT_RAMP_FIT_DTYPE)
        tab = np.zeros(K, dtype=SEGMENT_CELL_DTYPE) if cell_table else None
        sse = np.empty((S, A), dtype=np.float64) if curve else None
        plane = np.zeros((S, A), dtype=np.int8) if width_plane else None
        self._fit_call("sc_fit_segments_ramp", z, (cells, sa, ca), (seg_start, seg_label), ages,
                       [h, w, width, mode, slope, de, delta, min_samples, min_profiles, rows, tab, sse, plane])
        return rows, tab, sse, plane

    def fit_segments_robust(self, cells, sa, ca, seg_start, seg_label, ages, h, w, de, delta, min_samples, min_profiles,
                            weights=None, loss=ROBUST_NONE, tuning=0.0, iterations=1, scale=0.0, cell_table=False, curve=False,
                            z=None):
        """sc_fit_segments_robust on the context's DEM, or sc_fit_segments_robust_dem on ``z`` (float64, C-contiguous,
        2-D): (rows, cell table or None, (S, A) float64 loss curves or None).  The arrays as fit_segments takes them;
        ``weights``: None or a float64, C-contiguous plane of the DEM's shape; ``scale`` 0: estimated per segment."""
        self._check_weights(weights, z)
        K, A, S = len(cells), len(ages), len(seg_label)
        rows = np.zeros(S, dtype=SEGMENT_ROBUST_FIT_DTYPE)
        tab = np.zeros(K, dtype=SEGMENT_ROBUST_CELL_DTYPE) if cell_table else None
        out = np.empty((S, A), dtype=np.float64) if curve else None
        self._fit_call("sc_fit_segments_robust", z, (cells, sa, ca), (seg_start, seg_label), ages,
                       [h, w, de, delta, min_samples, min_profiles, weights, loss, tuning, iterations, scale, rows, tab, out])
        return rows, tab, out

    def fit_segments_refine(self, cells, sa, ca, seg_start, seg_label, ages, h, w, de, delta, min_samples, min_profiles,
                            refine, cell_table=False, curve=False, z=None):
        """sc_fit_segments_refine on the context's DEM, or sc_fit_segments_refine_dem on ``z`` (float64, C-contiguous,
        2-D): (rows, cell table or None, curve or None).  The arrays as fit_segments takes them; ``refine``: R, the
        levels of 64 candidate ages below the grid."""
        K, A, S = len(cells), len(ages), len(seg_label)
        rows = np.zeros(S, dtype=SEGMENT_FINE_FIT_DTYPE)
        tab = np.zeros(K, dtype=SEGMENT_FINE_CELL_DTYPE) if cell_table else None
        sse = np.empty((S, A), dtype=np.float64) if curve else None
        self._fit_call("sc_fit_segments_refine", z, (cells, sa, ca), (seg_start, seg_label), ages,
                       [h, w, refine, de, delta, min_samples, min_profiles, rows, tab, sse])
        return rows, tab, sse

    # -- block-bootstrap intervals per segment (docs/bootstrap.md) -----------------------
    def bootstrap_segments(self, cells, sa, ca, seg_start, seg_label, seg_blk_start, blk_start, ages, h, w, D, de,
                           min_samples, min_profiles, min_blocks, R, level, seed, hist=False, replicates=False, z=None):
        """sc_bootstrap_segments on the context's DEM, or sc_bootstrap_segments_dem on ``z`` (float64, C-contiguous,
        2-D): (rows, (S, A) int32 histograms or None, (S, R + 1) int8 indices or None, (S, R + 1) float64 amplitudes
        or None).  cells, seg_start, seg_blk_start and blk_start int64, seg_label int32, sa / ca / ages float64, all
        1-D and C-contiguous; the cells grouped by segment and, within it, by block."""
        A, S = len(ages), len(seg_label)
        assert len(seg_blk_start) == S + 1
        rows = np.zeros(S, dtype=SEGMENT_BOOT_DTYPE)
        hg = np.zeros((S, A), dtype=np.int32) if hist else None
        idx = np.zeros((S, int(R) + 1), dtype=np.int8) if replicates else None
        amp = np.zeros((S, int(R) + 1), dtype=np.float64) if replicates else None
        self._fit_call("sc_bootstrap_segments", z, (cells, sa, ca),
                       (seg_start, seg_label, seg_blk_start, blk_start, len(blk_start) - 1), ages,
                       [h, w, D, de, min_samples, min_profiles, min_blocks, R, level, seed, rows, hg, idx, amp])
        return rows, hg, idx, amp

    # -- block-bootstrap intervals per reach (docs/channels.md) --------------------------
    def channel_bootstrap(self, cells, sa, ca, seg_start, seg_label, seg_blk_start, blk_start, frequencies, h, w, D, mode, de,
                          min_samples, min_profiles, min_blocks, R, level, seed, hist=False, replicates=False, z=None):
        """sc_channel_bootstrap on the context's DEM, or sc_channel_bootstrap_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, (S, F) int32 histograms or None, (S, R + 1) int8 indices or None, (S, R + 1) float64 depth coefficients or
        None).  The arrays as bootstrap_segments takes them, the cells grouped by reach and, within it, by block; ``D``:
        the range of the centre shift in cells; ``mode``: CHANNEL_DEPTH_PROFILE or CHANNEL_DEPTH_SEGMENT."""
        F, S = len(frequencies), len(seg_label)
        assert len(seg_blk_start) == S + 1
        rows = np.zeros(S, dtype=CHANNEL_BOOT_DTYPE)
        hg = np.zeros((S, F), dtype=np.int32) if hist else None
        idx = np.zeros((S, int(R) + 1), dtype=np.int8) if replicates else None
        amp = np.zeros((S, int(R) + 1), dtype=np.float64) if replicates else None
        self._fit_call("sc_channel_bootstrap", z, (cells, sa, ca),
                       (seg_start, seg_label, seg_blk_start, blk_start, len(blk_start) - 1), frequencies,
                       [h, w, D, mode, de, min_samples, min_profiles, min_blocks, R, level, seed, rows, hg, idx, amp])
        return rows, hg, idx, amp

    # -- joint fits in windows along the strike (docs/strike.md) -------------------------
    def fit_strike(self, cells, sa, ca, seg_start, seg_label, seg_win_start, win_lo, win_hi, ages, h, w, D, de, delta,
                   min_samples, min_profiles, curve=False, z=None):
        """sc_fit_strike on the context's DEM, or sc_fit_strike_dem on ``z`` (float64, C-contiguous, 2-D): (rows, (NW, A)
        float64 curves or None).  cells, seg_start, seg_win_start, win_lo and win_hi int64, seg_label int32, sa / ca /
        ages float64, all 1-D and C-contiguous; the cells grouped by segment and sorted along its strike."""
        A, S, NW = len(ages), len(seg_label), len(win_lo)
        assert len(seg_win_start) == S + 1 and len(win_hi) == NW
        rows = np.zeros(NW, dtype=STRIKE_FIT_DTYPE)
        sse = np.empty((NW, A), dtype=np.float64) if curve else None
        self._fit_call("sc_fit_strike", z, (cells, sa, ca), (seg_start, seg_label, seg_win_start, win_lo, win_hi, NW), ages,
                       [h, w, D, de, delta, min_samples, min_profiles, rows, sse])
        return rows, sse

    # -- a channel's width in windows along the strike (docs/channels.md) -----------------
    def channel_strike(self, cells, sa, ca, seg_start, seg_label, seg_win_start, win_lo, win_hi, frequencies, h, w, D, mode,
                       de, delta, min_samples, min_profiles, curve=False, z=None):
        """sc_channel_strike on the context's DEM, or sc_channel_strike_dem on ``z`` (float64, C-contiguous, 2-D): (rows,
        (NW, F) float64 curves or None, (NW,) int32 sums of the shifts).  The arrays as fit_strike takes them, the cells
        grouped by reach and sorted along its strike; ``D``: the range of the centre shift in cells; ``mode``:
        CHANNEL_DEPTH_PROFILE or CHANNEL_DEPTH_SEGMENT.  The rows are sc_strike_fit, kt carrying f (docs/channels.md)."""
        F, S, NW = len(frequencies), len(seg_label), len(win_lo)
        assert len(seg_win_start) == S + 1 and len(win_hi) == NW
        rows = np.zeros(NW, dtype=STRIKE_FIT_DTYPE)
        sse = np.empty((NW, F), dtype=np.float64) if curve else None
        shift_sum = np.zeros(NW, dtype=np.int32)
        self._fit_call("sc_channel_strike", z, (cells, sa, ca), (seg_start, seg_label, seg_win_start, win_lo, win_hi, NW),
                       frequencies, [h, w, D, mode, de, delta, min_samples, min_profiles, rows, sse, shift_sum])
        return rows, sse, shift_sum

    # -- block-bootstrap intervals per station (docs/strike.md) --------------------------
    def strike_bootstrap(self, cells, sa, ca, seg_start, seg_label, seg_win_start, win_lo, win_hi, win_blk_start, blk_hi,
                         ages, h, w, D, de, min_samples, min_profiles, min_blocks, R, level, seed, hist=False, z=None):
        """sc_strike_bootstrap on the context's DEM, or sc_strike_bootstrap_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, (NW, A) int32 histograms or None).  cells, seg_start, seg_win_start, win_lo, win_hi, win_blk_start and
        blk_hi int64, seg_label int32, sa / ca / ages float64, all 1-D and C-contiguous; the cells grouped by segment and
        sorted along its strike."""
        A, S, NW = len(ages), len(seg_label), len(win_lo)
        assert len(seg_win_start) == S + 1 and len(win_hi) == NW and len(win_blk_start) == NW + 1
        for a in (win_blk_start, blk_hi):
            assert a.dtype == np.int64 and a.ndim == 1 and a.flags.c_contiguous
        rows = np.zeros(NW, dtype=STRIKE_BOOT_DTYPE)
        hg = np.zeros((NW, A), dtype=np.int32) if hist else None
        self._fit_call("sc_strike_bootstrap", z, (cells, sa, ca), (seg_start, seg_label, seg_win_start, win_lo, win_hi, NW), ages,
                       [h, w, D, de, min_samples, min_profiles, win_blk_start, blk_hi, len(blk_hi), min_blocks, R, level, seed,
                        rows, hg])
        return rows, hg

    # -- block-bootstrap intervals per station along a reach (docs/channels.md) ------------
    def channel_strike_bootstrap(self, cells, sa, ca, seg_start, seg_label, seg_win_start, win_lo, win_hi, win_blk_start, blk_hi,
                                 frequencies, h, w, D, mode, de, min_samples, min_profiles, min_blocks, R, level, seed, hist=False,
                                 z=None):
        """sc_channel_strike_bootstrap on the context's DEM, or sc_channel_strike_bootstrap_dem on ``z`` (float64,
        C-contiguous, 2-D): (rows, (NW, F) int32 histograms or None).  The arrays as strike_bootstrap takes them, the cells
        grouped by reach and sorted along its strike; ``D``: the range of the centre shift in cells; ``mode``:
        CHANNEL_DEPTH_PROFILE or CHANNEL_DEPTH_SEGMENT."""
        F, S, NW = len(frequencies), len(seg_label), len(win_lo)
        assert len(seg_win_start) == S + 1 and len(win_hi) == NW and len(win_blk_start) == NW + 1
        for a in (win_blk_start, blk_hi):
            assert a.dtype == np.int64 and a.ndim == 1 and a.flags.c_contiguous
        rows = np.zeros(NW, dtype=CHANNEL_STRIKE_BOOT_DTYPE)
        hg = np.zeros((NW, F), dtype=np.int32) if hist else None
        self._fit_call("sc_channel_strike_bootstrap", z, (cells, sa, ca),
                       (seg_start, seg_label, seg_win_start, win_lo, win_hi, NW), frequencies,
                       [h, w, D, mode, de, min_samples, min_profiles, win_blk_start, blk_hi, len(blk_hi), min_blocks, R, level,
                        seed, rows, hg])
        return rows, hg

    # -- strike-slip offsets across a trace (docs/lateral.md) -------------------------------
    def lateral_offsets(self, cells, sa, ca, h, q0, q1, D, de, delta, min_samples, curve=False, z=None):
        """sc_lateral_offsets on the context's DEM, or sc_lateral_offsets_dem on ``z`` (float64, C-contiguous, 2-D):
        (rows, (K, 2 D + 1) float64 mse curves or None).  cells int64, sa / ca float64, all 1-D and C-contiguous."""
        K = len(cells)
        rows = np.zeros(K, dtype=LATERAL_FIT_DTYPE)
        mse = np.empty((K, 2 * int(D) + 1), dtype=np.float64) if curve else None
        self._fit_call("sc_lateral_offsets", z, (cells, sa, ca), None, None, [h, q0, q1, D, de, delta, min_samples, rows, mse])
        return rows, mse

    # -- the SNR surface at chosen cells (docs/surface.md) ---------------------------------
    def snr_surface(self, templates, n_par, n_ang, cells, keep, surface=False):
        """sc_snr_surface on the context's DEM: (rows, snr, amp).  ``templates``: the n_par * n_ang descriptors of
        Matcher.describe (orientation-major); ``cells``: (K, 2) int32 (row, col); ``keep`` = 1 - drop.  With ``surface`` the
        two (K, n_ang, n_par) float64 cubes, else None.  The record stays; the scorers' last search is this table after."""
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
        K = len(cells)
        assert len(templates) == int(n_par) * int(n_ang)
        rows = np.zeros(K, dtype=SURFACE_ROW_DTYPE)
        snr = np.empty((K, int(n_ang), int(n_par)), dtype=np.float64) if surface else None
        amp = np.empty((K, int(n_ang), int(n_par)), dtype=np.float64) if surface else None
        self._check(self.lib.sc_snr_surface(self._h, templates, int(n_par), int(n_ang), cells.ctypes.data_as(C.POINTER(C.c_int32)),
                                            K, float(keep), rows.ctypes.data_as(C.c_void_p),
                                            _as(snr, _dp) if surface else None, _as(amp, _dp) if surface else None),
                    "sc_snr_surface")
        return rows, snr, amp

    # -- measurement ----------------------------------------------------------
    def profile(self, stride):
        self._check(self.lib.sc_profile(self._h, int(stride)), "sc_profile")

    def profile_get(self):
        out = {}
        for k, name in enumerate(K_NAMES):
            n = C.c_longlong(0)
            ms = C.c_double(0)
            self._check(self.lib.sc_profile_get(self._h, k, C.byref(n),
                                                C.byref(ms)), "sc_profile_get")
            out[name] = (n.value, ms.value)
        return out

    def device_bytes(self):
        return int(self.lib.sc_device_bytes(self._h))

    # -- multi-GPU ------------------------------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(COMM_ID_BYTES)
        rc = self.lib.sc_comm_unique_id(buf)
        if rc != SC_OK:
            raise ScarpletHipError("sc_comm_unique_id failed: %d" % rc)
        return buf.raw

    def comm_init(self, uid, rank, nranks):
        buf = C.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        self._check(self.lib.sc_comm_init(self._h, buf, rank, nranks),
                    "sc_comm_init")

    def near_ties(self):
        """(h, w) uint8: 1 where an FFT search since the last reset saw a near-tie (option "near_window")."""
        h, w = self.core_shape()
        out = np.zeros((h, w), dtype=np.uint8)
        self._check(self.lib.sc_get_near_ties(self._h, _as(out, _bp)), "sc_get_near_ties")
        return out

    def score_cells_f64(self, cells, n_templates):
        """(amp, snr) float64, each (m, n_templates): match_template() in float64 at the m global cells (rows of
        (i, j)) for every template of the last match in this context, in hand-over order (sc_score_cells_f64)."""
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
        m = len(cells)
        amp = np.empty((m, int(n_templates)), dtype=np.float64)
        snr = np.empty((m, int(n_templates)), dtype=np.float64)
        self._check(self.lib.sc_score_cells_f64(self._h, cells.ctypes.data_as(C.POINTER(C.c_int32)), m, int(n_templates),
                                                _as(amp, _dp), _as(snr, _dp)), "sc_score_cells_f64")
        return amp, snr

    def near_events(self):
        """The near-ties of the searches since the last reset as events, (n, 4) uint32: cell (row-major index into the
        core planes), id of the template scored, id of the record's holder at that moment, float32 bits of the larger of
        their two scores (sc_get_near_events) - or None where the device list overflowed (more events than two per core cell)."""
        n = C.c_longlong(0)
        try:
            self._check(self.lib.sc_get_near_events(self._h, None, 0, C.byref(n)), "sc_get_near_events")
            want = int(n.value)
            if want == 0:
                return np.zeros((0, 4), dtype=np.uint32)
            ev = np.empty((want, 4), dtype=np.uint32)
            self._check(self.lib.sc_get_near_events(self._h, _as(ev, _up), want, C.byref(n)), "sc_get_near_events")
        except ScarpletHipError as e:
            if "overflowed" in str(e):                   # (the library says so itself since ABI 8)
                return None
            raise
        if int(n.value) != want:
            return None
        return ev

    def score_pairs_f64(self, cells, templates):
        """(amp, snr) float64, each (m,): match_template() in float64 at global cell cells[k] for template templates[k]
        (index in the last match's hand-over order) - sc_score_pairs_f64."""
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
        templates = np.ascontiguousarray(templates, dtype=np.int32).reshape(-1)
        m = len(cells)
        amp = np.empty(m, dtype=np.float64)
        snr = np.empty(m, dtype=np.float64)
        i32 = C.POINTER(C.c_int32)
        self._check(self.lib.sc_score_pairs_f64(self._h, cells.ctypes.data_as(i32), templates.ctypes.data_as(i32), m,
                                                _as(amp, _dp), _as(snr, _dp)), "sc_score_pairs_f64")
        return amp, snr

    def settle_exact(self, n_twin=0, max_work=0.0):
        """exact=True on the device (sc_settle_exact): the near-tie cells of the last search (option "near_window") take
        their float64 argmax among the templates their events name.  Returns the counters as a dict."""
        st = (C.c_longlong * 8)()
        self._check(self.lib.sc_settle_exact(self._h, int(n_twin), float(max_work), st), "sc_settle_exact")
        return self._settle_stats(st)

    @staticmethod
    def _settle_stats(st):
        """The settle's counters as a dict.  ``max_f32_err``: the audit (stats[6], units of 1e-9) - the largest relative
        error of a scored record holder's float32 SNR against its float64 score: a lower bound on the search's error."""
        return {"flagged_cells": int(st[0]), "pairs_listed": int(st[1]), "float64_pairs": int(st[2]),
                "float64_cells": int(st[3]), "changed_cells": int(st[4]), "events": int(st[5]),
                "max_f32_err": int(st[6]) * 1e-9, "taps": int(st[7])}

    # ---- exact mode of an orientation-sharded search (include/scarplet_hip.h: sc_settle_pairs) ----
    def snapshot_best(self):
        """Keep the record's (snr, id) planes as they stand on the device - before the fold over the ranks."""
        self._check(self.lib.sc_snapshot_best(self._h), "sc_snapshot_best")

    def set_best(self, amp, snr, idx):
        """Upload a record (core-shaped float32, float32, uint32) as the running best (sc_set_best)."""
        h, w = self.core_shape()
        amp = np.ascontiguousarray(amp, dtype=np.float32)
        snr = np.ascontiguousarray(snr, dtype=np.float32)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        if not (amp.shape == snr.shape == idx.shape == (h, w)):
            raise ValueError("set_best: the record must have the core's shape %r" % ((h, w),))
        self._check(self.lib.sc_set_best(self._h, _as(amp, _fp), _as(snr, _fp), _as(idx, _up)), "sc_set_best")

    def rank_candidates(self, fetch=True):
        """This rank's candidates against the folded record: an (n, 2) uint32 array of (core cell index, template id)
        (sc_rank_candidates: the templates of this rank's events and its own holder that lie within the near-tie window
        of the record as it stands now).  ``fetch=False``: the list stays on the device (exchange_candidates), the count
        is returned."""
        n = C.c_longlong(0)
        self._check(self.lib.sc_rank_candidates(self._h, None, 0, C.byref(n)), "sc_rank_candidates")
        if not fetch:
            return n.value
        out = np.empty((n.value, 2), dtype=np.uint32)
        if n.value:
            m = C.c_longlong(0)
            self._check(self.lib.sc_rank_candidates(self._h, _as(out, _up), n.value, C.byref(m)), "sc_rank_candidates")
            if m.value != n.value:
                raise ScarpletHipError("sc_rank_candidates: %d pairs, then %d" % (n.value, m.value))
        return out

    def exchange_candidates(self):
        """All ranks' candidate lists as one list on every device (sc_exchange_candidates: two all-gathers over RCCL);
        returns its length in pairs, padding included - what settle_pairs(templates, None, ...) then settles."""
        n = C.c_longlong(0)
        self._check(self.lib.sc_exchange_candidates(self._h, C.byref(n)), "sc_exchange_candidates")
        self._exchanged = n.value
        return n.value

    def settle_pairs(self, templates, pairs, n_twin=0, max_work=0.0):
        """Settle the union of all ranks' candidates with the descriptors of the WHOLE search (sc_settle_pairs); the
        counters as settle_exact returns them.  ``pairs``: an (n, 2) uint32 array, or None for the list
        exchange_candidates left on the device."""
        if any(int(t.kind) == KIND_WINDOW for t in templates):
            # (the library refuses them as well: another rank's window slots do not exist in this context)
            raise ScarpletHipError("sc_settle_pairs: templates with host-uploaded windows (generic plugins) are not settled "
                                   "across ranks - the orientation-sharded exact mode takes the built-in template classes only")
        st = (C.c_longlong * 8)()
        if pairs is None:
            ptr, n = None, int(getattr(self, "_exchanged", 0))
        else:
            pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
            ptr, n = (_as(pairs, _up) if len(pairs) else None), len(pairs)
        self._check(self.lib.sc_settle_pairs(self._h, templates, len(templates), ptr, n, int(n_twin), float(max_work), st),
                    "sc_settle_pairs")
        return self._settle_stats(st)

    def comm_destroy(self):
        """Drop this context's RCCL communicator (sc_comm_destroy); nothing to do without one."""
        self._check(self.lib.sc_comm_destroy(self._h), "sc_comm_destroy")

    def resolution_stats(self):
        """(wins, wins near the float32 resolution floor) of the FFT searches since the last
        reset_best (sc_get_resolution_stats)."""
        a, b = C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.sc_get_resolution_stats(self._h, C.byref(a), C.byref(b)), "sc_get_resolution_stats")
        return a.value, b.value

    def comm_info(self):
        """What RCCL reports for this context's communicator (sc_comm_info): a dict with
        nranks (0: no communicator), rank, device and the device's PCI bus id."""
        n, r, d = C.c_int(0), C.c_int(-1), C.c_int(-1)
        bus = C.create_string_buffer(32)
        self._check(self.lib.sc_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d), bus, 32), "sc_comm_info")
        return {"nranks": n.value, "rank": r.value, "device": d.value, "bus_id": bus.value.decode()}

    def fold_ranks(self):
        """Collective fold of the ranks' running-best records (orientation-sharded search)."""
        self._check(self.lib.sc_fold_ranks(self._h), "sc_fold_ranks")

    def gather_result(self, root, cores, shape, param_of_id, angle_of_id, is_root, out=None):
        """Collective final gather over RCCL; returns (4, ny, nx) on root (``out``: a float64
        array of that shape to fill instead of a new one - the cores tile the DEM, every cell
        is written)."""
        cores = np.ascontiguousarray(cores, dtype=np.int32)
        par = np.ascontiguousarray(param_of_id, dtype=np.float64)
        ang = np.ascontiguousarray(angle_of_id, dtype=np.float64)
        if is_root and out is None:
            out = np.zeros((4,) + tuple(shape), dtype=np.float64)
        if is_root:
            assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (4,) + tuple(shape)
        self._check(self.lib.sc_gather_result(
            self._h, int(root), cores.ctypes.data_as(C.POINTER(C.c_int32)), int(shape[0]),
            int(shape[1]), _as(par, _dp), _as(ang, _dp), len(par),
            _as(out, _dp) if is_root else None), "sc_gather_result")
        return out

    def halo_exchange(self, core, halo, xfers):
        core = np.ascontiguousarray(core, dtype=np.float64)
        arr = (sc_xfer * max(len(xfers), 1))()
        for i, x in enumerate(xfers):
            arr[i] = sc_xfer(*[int(v) for v in x])
        z_dev = _P()
        self._check(self.lib.sc_halo_exchange(
            self._h, _as(core, _dp), core.shape[0], core.shape[1],
            int(halo[0]), int(halo[1]), int(halo[2]), int(halo[3]), arr,
            len(xfers), C.byref(z_dev)), "sc_halo_exchange")
        return z_dev
