"""The definition of docs/surface.md in numpy: the reduction of a (K, n_par, n_ang) SNR cube to sc_snr_surface's rows, and the
oracle's side of the comparisons - match_template() per template, its values at the cells, its largest values over the map.
Numpy only; the cases of tests/test_gpu_surface.py live here so that the CPU tests can stand on them too."""
import functools

import numpy as np

import scarplet_oracle as orc

ROW_FIELDS = [("par_index", np.int32), ("ang_index", np.int32), ("par_lo", np.int32), ("par_hi", np.int32),
              ("ang_lo", np.int32), ("ang_hi", np.int32), ("n_within", np.int32), ("status", np.int32),
              ("snr", np.float64), ("amp", np.float64)]


def reduce_cube(S, Amp, drop):
    """docs/surface.md applied to S, Amp of shape (K, n_par, n_ang): one row per cell (ROW_FIELDS).

    Templates are compared in hand-over order t = ib * n_par + ia; a NaN counts as -inf; the first maximum is the best.  No
    score > 0: status 1, indices -1, n_within 0, NaN floats.  thr = snr * (1.0 - drop), one multiply; P[ia] = max over ib,
    Q[ib] = max over ia; the walks go down and up from the best while the neighbour stays >= thr and do not wrap."""
    S = np.asarray(S, dtype=np.float64)
    Amp = np.asarray(Amp, dtype=np.float64)
    K, n_par, n_ang = S.shape
    keep = 1.0 - drop
    rows = np.zeros(K, dtype=np.dtype(ROW_FIELDS))
    C = np.where(np.isnan(S), -np.inf, S)
    flat = C.transpose(0, 2, 1).reshape(K, n_ang * n_par)                  # orientation-major, ages inner
    tbest = np.argmax(flat, axis=1)                                        # (numpy: the first maximum)
    Pm, Qm = C.max(axis=2), C.max(axis=1)
    for k in range(K):
        t = int(tbest[k])
        best = flat[k, t]
        r = rows[k]
        if not best > 0.0:
            r["par_index"] = r["ang_index"] = r["par_lo"] = r["par_hi"] = r["ang_lo"] = r["ang_hi"] = -1
            r["n_within"], r["status"] = 0, 1
            r["snr"] = r["amp"] = np.nan
            continue
        ib, ia = divmod(t, n_par)
        thr = best * keep
        P, Q = Pm[k], Qm[k]
        plo = phi = ia
        alo = ahi = ib
        while plo > 0 and P[plo - 1] >= thr:
            plo -= 1
        while phi < n_par - 1 and P[phi + 1] >= thr:
            phi += 1
        while alo > 0 and Q[alo - 1] >= thr:
            alo -= 1
        while ahi < n_ang - 1 and Q[ahi + 1] >= thr:
            ahi += 1
        r["par_index"], r["ang_index"] = ia, ib
        r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"] = plo, phi, alo, ahi
        r["n_within"] = int(np.count_nonzero(C[k] >= thr))
        r["status"] = (2 if plo == 0 else 0) + (4 if phi == n_par - 1 else 0) + (8 if alo == 0 else 0) + \
            (16 if ahi == n_ang - 1 else 0)
        r["snr"], r["amp"] = best, Amp[k, ia, ib]
    return rows


def table_rows(tab):
    """The Python table of sl.snr_surface back as library rows (ROW_FIELDS), for bitwise comparison with reduce_cube."""
    rows = np.zeros(len(tab), dtype=np.dtype(ROW_FIELDS))
    for dst, src in (("par_index", "par_index"), ("ang_index", "ang_index"), ("par_lo", "par_lo_index"),
                     ("par_hi", "par_hi_index"), ("ang_lo", "ang_lo_index"), ("ang_hi", "ang_hi_index"),
                     ("n_within", "n_within"), ("status", "status"), ("snr", "snr"), ("amp", "amp")):
        rows[dst] = tab[src]
    return rows


# ---- the cases of the GPU comparisons -------------------------------------------------------------------------------------
def _noise(rng, ny, nx):
    return (np.cumsum(np.cumsum(rng.standard_normal((ny, nx)), 0), 1) * 0.01 + rng.standard_normal((ny, nx)) * 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(z, de, dy, kind, cls (name of the class in scarplet_amd), scale, params, angles).  The surfaces of A, B,
    C, D and F are drawn from ONE default_rng(33), in that order."""
    rng = np.random.default_rng(33)
    spec = [("A", 90, 101, 1.0, 1.0, orc.SCARP, "Scarp", 8, [1.0, 6.0, 40.0], [-1.3, -0.2, 0.0, 0.9, np.pi / 2]),
            ("B", 80, 64, 2.0, -2.0, orc.SCARP, "Scarp", 14, [3.0, 25.0], [-np.pi / 2, 0.4]),
            ("C", 72, 76, 1.0, 1.0, "left_upper_break", "LeftFacingUpperBreakScarp", 9, [5.0], [-0.6, 0.7]),
            ("D", 64, 72, 1.0, -1.0, orc.RICKER, "Ricker", 6, [0.1, 0.25], [-0.8, 0.0, 1.1]),
            ("F", 160, 176, 1.0, 1.0, orc.SCARP, "Scarp", 40, [100.0, 200.0, 400.0, 800.0, 1600.0], [0.0, 0.7, -1.4])]
    out = {}
    for name, ny, nx, de, dy, kind, cls, scale, params, angles in spec:
        out[name] = dict(z=_noise(rng, ny, nx), de=de, dy=dy, kind=kind, cls=cls, scale=scale,
                         params=np.asarray(params, dtype=np.float64), angles=np.asarray(angles, dtype=np.float64))
    out["E"] = dict(z=orc.synthetic_dem(96), de=1.0, dy=1.0, kind=orc.SCARP, cls="Scarp", scale=10,
                    params=10 ** np.arange(0, 2, 0.25), angles=np.linspace(-np.pi / 2, np.pi / 2, 13)[:-1])
    return out


@functools.lru_cache(maxsize=None)
def oracle_cubes(name):
    """The oracle at ALL cells of case ``name``: (S, Amp) of shape (ny * nx, n_par, n_ang), cells row-major, and per
    template its largest SNR and largest |amp| over the whole map, (n_par, n_ang) each.  Computed once per process."""
    c = cases()[name]
    z = c["z"]
    ny, nx = z.shape
    n_par, n_ang = len(c["params"]), len(c["angles"])
    S = np.empty((ny * nx, n_par, n_ang))
    A = np.empty((ny * nx, n_par, n_ang))
    for ib, ang in enumerate(c["angles"]):
        for ia, par in enumerate(c["params"]):
            amp, _, _, snr = orc.match_template(z, c["de"], c["dy"], c["kind"], c["scale"], float(par), float(ang))
            S[:, ia, ib] = snr.ravel()
            A[:, ia, ib] = amp.ravel()
    for v in (S, A):
        v.setflags(write=False)
    return S, A, S.max(axis=0), np.abs(A).max(axis=0)


def oracle_ties(name):
    """(live, excluded, first): the cells whose top oracle score is > 0, those of them whose two top scores differ by at
    most 2e-9 * M (M: the largest oracle SNR of any template of the case), and the oracle's first maximum per cell as
    (ia, ib) in hand-over order."""
    S, _, smax, _ = oracle_cubes(name)
    K, n_par, n_ang = S.shape
    flat = np.where(np.isnan(S), -np.inf, S).transpose(0, 2, 1).reshape(K, -1)
    t = np.argmax(flat, axis=1)
    top = flat[np.arange(K), t]
    live = top > 0
    if flat.shape[1] > 1:
        second = np.partition(flat, -2, axis=1)[:, -2]
    else:
        second = np.full(K, -np.inf)
    excluded = live & (top - second <= 2e-9 * smax.max())
    return live, excluded, (t % n_par, t // n_par)
