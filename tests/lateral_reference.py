"""sl.lateral_offsets restated in plain numpy (docs/lateral.md), and the synthetic surfaces its tests share.

The restatement follows the definition to the letter: the sample positions, the bilinear weights, the order of every sum
(``_seq``: a running sum from +0.0, an invalid term a +0.0 that changes nothing), the candidates' order, the walk and the
parabola.  It uses +, -, *, / and sqrt alone, as the device does, so the two differ by no more than a compiler may
differ from numpy; the tests allow 1e-9 relative."""
import numpy as np

FIELDS = [("row", np.int64), ("col", np.int64), ("cell", np.int64), ("n", np.int32), ("lag", np.int32), ("lo", np.int32),
          ("hi", np.int32), ("status", np.int32), ("offset", np.float64), ("offset_lo", np.float64),
          ("offset_hi", np.float64), ("mse", np.float64), ("rho", np.float64), ("dz", np.float64), ("tilt", np.float64)]
INT_FIELDS = ("row", "col", "cell", "n", "lag", "lo", "hi", "status")
FLOAT_FIELDS = ("offset", "offset_lo", "offset_hi", "mse", "rho", "dz", "tilt")


def shift_of(r):
    """Rank r -> lag, in the order 0, -1, +1, -2, +2, ..."""
    return -((r + 1) >> 1) if r & 1 else r >> 1


def _seq(x, axis=-1):
    """The sum of x along ``axis`` in ascending order, one addition at a time, from +0.0."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    x = np.concatenate([np.zeros(x.shape[:-1] + (1,)), x], axis=-1)
    return np.cumsum(x, axis=-1)[..., -1]


def sample(z, rr, cc):
    """Bilinear samples of z at (rr, cc) and whether each is valid: inside the grid and finite."""
    ny, nx = z.shape
    with np.errstate(invalid="ignore"):
        inside = (rr >= 0.0) & (rr <= float(ny - 1)) & (cc >= 0.0) & (cc <= float(nx - 1))
    rs, cs = np.where(inside, rr, 0.0), np.where(inside, cc, 0.0)
    r0 = np.minimum(np.floor(rs).astype(np.int64), ny - 2)
    c0 = np.minimum(np.floor(cs).astype(np.int64), nx - 2)
    fr, fc = rs - r0, cs - c0
    z00, z01, z10, z11 = z[r0, c0], z[r0, c0 + 1], z[r0 + 1, c0], z[r0 + 1, c0 + 1]
    with np.errstate(invalid="ignore"):
        v = (z00 * (1.0 - fc) + z01 * fc) * (1.0 - fr) + (z10 * (1.0 - fc) + z11 * fc) * fr
    return v, inside & np.isfinite(v)


def side(z, r, c, sa, ca, t, qs):
    """The profile over the along-strike indices ``t`` of the band of lines ``qs`` (signed, in the order of the sum)."""
    t = np.asarray(t, dtype=np.float64)
    q = np.asarray(qs, dtype=np.float64)[None, :]
    tca, tsa = (t * ca)[:, None], (t * sa)[:, None]
    rr = float(r) + (tca - q * sa)
    cc = float(c) + (q * ca + tsa)
    v, ok = sample(z, rr, cc)
    acc = _seq(np.where(ok, v, 0.0), axis=1)
    cnt = ok.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, acc / cnt, np.nan)


def profiles(z, r, c, sa, ca, h, q0, q1, D):
    """(u over t = -h..h on the -q side, v over t = -(h + D)..(h + D) on the +q side)."""
    qs = np.arange(q0, q1 + 1)
    return (side(z, r, c, sa, ca, np.arange(-h, h + 1), -qs),
            side(z, r, c, sa, ca, np.arange(-(h + D), h + D + 1), qs))


def curves(u, v, h, D, de, min_samples):
    """Every lag at once, row d + D: (fitted, n, mse, rho, dz, tilt)."""
    npts, nl = 2 * h + 1, 2 * D + 1
    vd = np.lib.stride_tricks.sliding_window_view(v, npts)              # vd[d + D, t + h] = v_{t + d}
    assert vd.shape == (nl, npts)
    ok = ~np.isnan(u)[None, :] & ~np.isnan(vd)
    s = np.arange(-h, h + 1).astype(np.float64) * de
    U = np.broadcast_to(u, vd.shape)
    S = np.broadcast_to(s, vd.shape)
    tot = lambda x: _seq(np.where(ok, x, 0.0), axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = ok.sum(axis=1)
        dn = n.astype(np.float64)
        sbar, ubar, vbar = tot(S) / dn, tot(U) / dn, tot(vd) / dn
        sc = S - sbar[:, None]
        uc, vc = U - ubar[:, None], vd - vbar[:, None]
        Stt, Stu, Stv = tot(sc * sc), tot(sc * uc), tot(sc * vc)
        bu, bv = Stu / Stt, Stv / Stt
        ru = uc - bu[:, None] * sc
        rv = vc - bv[:, None] * sc
        dr = rv - ru
        Suu, Svv, Suv, sse = tot(ru * ru), tot(rv * rv), tot(ru * rv), tot(dr * dr)
        fitted = (n >= min_samples) & (Stt > 0.0)
        mse = np.where(fitted, sse / (dn - 2.0), np.nan)
        den = Suu * Svv
        rho = np.where(fitted & (den > 0.0), Suv / np.sqrt(den), np.nan)
        dz = np.where(fitted, vbar - ubar, np.nan)
        tilt = np.where(fitted, bv - bu, np.nan)
    return fitted, n, mse, rho, dz, tilt


def station(z, cell, sa, ca, h, q0, q1, D, de, delta, min_samples):
    """One station: (the row's fields as a dict, the mse curve over d = -D..D)."""
    nx = z.shape[1]
    r, c = int(cell) // nx, int(cell) % nx
    u, v = profiles(z, r, c, sa, ca, h, q0, q1, D)
    fitted, n, mse, rho, dz, tilt = curves(u, v, h, D, de, min_samples)
    row = dict(row=r, col=c, cell=int(cell), n=0, lag=0, lo=0, hi=0, status=1)
    row.update({f: np.nan for f in FLOAT_FIELDS})
    best = None
    for rk in range(2 * D + 1):
        i = shift_of(rk) + D
        if fitted[i] and mse[i] == mse[i] and (best is None or mse[i] < mse[best]):
            best = i
    if best is None:
        return row, mse
    lag, m0, nb = best - D, mse[best], int(n[best])
    thr = m0 * (1.0 + delta / float(nb - 2))
    lo = hi = lag
    while lo > -D and mse[lo - 1 + D] <= thr:
        lo -= 1
    while hi < D and mse[hi + 1 + D] <= thr:
        hi += 1
    frac = 0.0
    if -D < lag < D:
        mm, mp = mse[best - 1], mse[best + 1]
        den = (mm - m0) + (mp - m0)
        if np.isfinite(mm) and np.isfinite(mp) and den > 0.0:
            frac = 0.5 * (mm - mp) / den
    status = (2 if lo == -D else 0) + (4 if hi == D else 0) + (8 if D > 0 and abs(lag) == D else 0) \
        + (16 if not fitted.all() else 0)
    row.update(n=nb, lag=lag, lo=lo, hi=hi, status=status, offset=(float(lag) + frac) * de, offset_lo=float(lo) * de,
               offset_hi=float(hi) * de, mse=m0, rho=rho[best], dz=dz[best], tilt=tilt[best], thr=thr)
    return row, mse


def lateral_offsets(z, de, cells, angle, h, q0, q1, D, delta=1.0, min_samples=8):
    """(table, (K, 2 D + 1) mse curves, thr per station - NaN where not fitted): h, q0, q1, D in cells."""
    z = np.asarray(z, dtype=np.float64)
    cells = np.atleast_1d(np.asarray(cells, dtype=np.int64))
    a = np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape)
    sa, ca = np.sin(a), np.cos(a)
    out = np.zeros(len(cells), dtype=np.dtype(FIELDS))
    mse = np.full((len(cells), 2 * D + 1), np.nan)
    thr = np.full(len(cells), np.nan)
    for k, cell in enumerate(cells):
        row, mse[k] = station(z, cell, sa[k], ca[k], h, q0, q1, D, float(de), float(delta), int(min_samples))
        thr[k] = row.pop("thr", np.nan)
        for f, val in row.items():
            out[f][k] = val
    return out, mse, thr


# ---- the planted surface ------------------------------------------------------------------------------------------------------
PLANT_SHAPE = (200, 240)
PLANT_S = 7.3
PLANT = dict(h=40, q0=2, q1=6, D=20)                                    # in cells, de = 1
PLANT_THETAS = (0.3, -1.1, 0.3 + np.pi)


def planted_surface(theta, s=PLANT_S, noise=0.02, seed=3):
    """A strike-slip fault through the centre of a 200 x 240 grid, strike ``theta``: 40 Gaussian ridges and troughs
    across it (amplitudes in +-1, widths 2 to 6 cells, irregular positions) displaced by ``s`` cells along the strike on
    the +Q side, which also stands 0.5 higher and tilts by 0.003 along the strike; 0.02 Q everywhere, Gaussian noise."""
    ny, nx = PLANT_SHAPE
    rng = np.random.default_rng(seed)
    amp = rng.uniform(-1.0, 1.0, 40)
    wid = rng.uniform(2.0, 6.0, 40)
    pos = rng.uniform(-150.0, 150.0, 40)
    f = lambda T: (amp * np.exp(-0.5 * ((T[..., None] - pos) / wid) ** 2)).sum(axis=-1)
    r, c = np.mgrid[0:ny, 0:nx].astype(np.float64)
    r0, c0 = ny // 2, nx // 2
    T = (r - r0) * np.cos(theta) + (c - c0) * np.sin(theta)
    Q = -(r - r0) * np.sin(theta) + (c - c0) * np.cos(theta)
    z = np.where(Q <= 0.0, f(T), f(T - s) + 0.5 + 0.003 * T)
    return z + 0.02 * Q + noise * rng.standard_normal((ny, nx))


def planted_stations(theta, n=11, step=5.0):
    """n cells along the fault's line, ``step`` apart, about the centre."""
    ny, nx = PLANT_SHAPE
    k = (np.arange(n) - (n - 1) / 2.0) * step
    r = np.rint(ny // 2 + k * np.cos(theta)).astype(np.int64)
    c = np.rint(nx // 2 + k * np.sin(theta)).astype(np.int64)
    return r * nx + c


# ---- the small DEMs of the device tests ---------------------------------------------------------------------------------------
def rough_dem(shape, seed):
    """Smooth relief and unit noise, a block and a sprinkle of NaN cells."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:ny, 0:nx].astype(np.float64)
    z = 3.0 * np.sin(r / 7.0) * np.cos(c / 5.0) + 0.05 * r - 0.03 * c + rng.standard_normal(shape)
    z[ny // 3:ny // 3 + 4, nx // 2:nx // 2 + 6] = np.nan
    z.ravel()[rng.choice(ny * nx, 25, replace=False)] = np.nan
    return z


def rough_stations(shape, K, seed):
    """K cells: the corners, cells on the borders, cells of the interior and repeats."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    fixed = [0, nx - 1, (ny - 1) * nx, ny * nx - 1, nx // 2, (ny // 2) * nx, (ny // 2) * nx + nx - 1, (ny - 1) * nx + nx // 3,
             (ny // 2) * nx + nx // 2, (ny // 2) * nx + nx // 2]
    if K <= 5:
        return np.array(([(ny // 2) * nx + nx // 2] + fixed)[:K], dtype=np.int64)
    rest = rng.integers(0, ny * nx, K - len(fixed))
    rest[-3:] = rest[:3]
    return np.concatenate([fixed, rest]).astype(np.int64)
