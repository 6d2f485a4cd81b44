"""exact=True for templates whose windows the host uploads (SC_KIND_WINDOW: the Shifted classes, any user plugin).

The reference folds float64 SNR maps for every template class (compare(), core.py:230-240; the serial driver, core.py:65-136,
is the only route to the Shifted classes).  The device keeps every uploaded window in float64 next to its float32 copy and
the settle scores those windows with the search orientation's curvature and the plugin's per-cell masks; its audit
(exact_stats["max_f32_err"]) measures the float32 error of every search.  Checked here against the oracle's float64
match_template() (orc.match_arrays over the plugin's own arrays) and against the reference's serial-driver capture."""
import time

import numpy as np
import pytest

import scarplet_oracle as orc
import scarplet_amd as sl
from scarplet_amd import WindowedTemplate as WT
from scarplet_amd import _plan
from conftest import golden

pytestmark = pytest.mark.gpu

TWIN = 1e-9                     # orc.check_fold's twin rule: two templates whose float64 SNRs agree to this are one maximum


def grid(z, de):
    return sl.DEMGrid.from_array(np.asarray(z, dtype=np.float32), de)


def _stack(z, dx, dy, make, params, angles):
    """The oracle's float64 (amp, snr) of every template, orientation-major (the order of Matcher.describe)."""
    amps, snrs = [], []
    for ang in angles:
        curv = orc.directional_curvature(z, dx, dy, ang)
        for par in params:
            t = make(par, ang)
            err = np.asarray(t.get_err_mask(), dtype=bool) if hasattr(t, "get_err_mask") else None
            a, s = orc.match_arrays(curv, np.asarray(t.template(), dtype=float),
                                    np.asarray(t.get_window_limits(), dtype=bool), err)
            amps.append(a)
            snrs.append(s)
    return np.stack(amps), np.stack(snrs)


def _template_index(res, params, angles):
    """Per cell the index (orientation-major) of the template the result holds; -1 where it holds none."""
    ia = np.abs(np.asarray(res[1])[..., None] - np.asarray(params)).argmin(-1)
    ib = np.abs(np.asarray(res[2])[..., None] - np.asarray(angles)).argmin(-1)
    k = ib * len(params) + ia
    ok = np.isclose(np.asarray(res[1]), np.asarray(params)[ia], rtol=1e-12, atol=0) & \
        (np.asarray(res[2]) == np.asarray(angles)[ib])
    return np.where(ok & (np.asarray(res[3]) > 0), k, -1)


def _off_argmax(res, snr_stack, params, angles):
    """Cells whose record is not the oracle's float64 argmax (the twin rule applied): count and where."""
    k = _template_index(res, params, angles)
    top = snr_stack.max(0)
    held = np.take_along_axis(snr_stack, np.maximum(k, 0)[None], 0)[0]
    won = (k >= 0) & (held >= top * (1 - TWIN))
    masked = (top == 0) & (np.asarray(res[3]) == 0)
    bad = ~(won | masked)
    return int(bad.sum()), bad


# ---- a plugin whose neighbouring "ages" differ by a millionth of their shape ----------------------------------------
_RNG = np.random.default_rng(20261015)
_BASE = _RNG.standard_normal((9, 11))
_PERT = _RNG.standard_normal((9, 11))
_HOLES = _RNG.random((9, 11)) < 0.2             # a support with holes: the settle's row runs must skip them
_BASE[_HOLES] = 0.0
_PERT[_HOLES] = 0.0


class NearTiePlugin(object):
    """Not a built-in twin (WT.builtin_twin: None): template() is uploaded.  W = base + age * 1e-6 * perturbation - the
    float32 SNRs of neighbouring ages lie inside float32 rounding of each other, their float64 SNRs far outside 1e-9.
    Its ``alpha`` is deliberately NOT the orientation: the curvature must be mixed with the search orientation's."""

    def __init__(self, d, age, angle, nx, ny, de):
        self.d, self.age, self.angle, self.nx, self.ny, self.de = d, age, angle, nx, ny, de
        self.alpha = 0.3 - angle

    def template(self):
        W = np.zeros((self.ny, self.nx))
        cy, cx = self.ny // 2, self.nx // 2
        W[cy - 4:cy + 5, cx - 5:cx + 6] = _BASE + (self.age * 1e-6) * _PERT
        return W

    def get_window_limits(self):
        return np.zeros((self.ny, self.nx), dtype=bool)


class NearTieMaskedPlugin(NearTiePlugin):
    """The same windows with per-cell masks: a ragged border and scattered cells of get_window_limits() (amp and snr 0),
    an orientation-dependent get_err_mask() (snr 0).  The FFT row kernel cannot flag these: the real-space route."""

    def get_window_limits(self):
        rng = np.random.default_rng(3)
        lim = rng.random((self.ny, self.nx)) < 0.03
        lim[:6, :] = lim[-5:, :] = True
        lim[:, :7] = lim[:, -6:] = True
        lim[40:44, 30:35] = True
        return lim

    def get_err_mask(self):
        rng = np.random.default_rng(5000 + int(round(1000 * self.angle)))
        return rng.random((self.ny, self.nx)) < 0.05


PLUGIN_AGES = [1.0, 2.0, 3.0, 4.0, 5.0]
PLUGIN_ANGLES = [-1.0, -0.2, 0.6, 1.3]


@pytest.fixture(scope="module")
def noise_dem():
    rng = np.random.default_rng(42)
    shape = (192, 200)
    z = (np.cumsum(rng.standard_normal(shape), 1) * 0.05 + rng.standard_normal(shape) * 0.03).astype(np.float32)
    return z


def _plugin_oracle(z, cls):
    ny, nx = z.shape
    return _stack(np.asarray(z, dtype=float), 1.0, 1.0, lambda par, ang: cls(10.0, par, ang, nx, ny, 1.0),
                  PLUGIN_AGES, PLUGIN_ANGLES)


@pytest.fixture(scope="module")
def oracle_plain(noise_dem):
    return _plugin_oracle(noise_dem, NearTiePlugin)


@pytest.fixture(scope="module")
def oracle_masked(noise_dem):
    return _plugin_oracle(noise_dem, NearTieMaskedPlugin)


def test_plugin_is_generic_and_float32_cannot_decide(noise_dem, oracle_plain):
    """The premise: the plugin takes the uploaded-window path, and its ages' float64 SNRs differ by far more than the twin
    rule but by less than float32 resolves."""
    assert WT.builtin_twin(NearTiePlugin) is None
    _, snr = oracle_plain
    s = snr.reshape(len(PLUGIN_ANGLES), len(PLUGIN_AGES), *snr.shape[1:])
    top = s.max(1)
    live = top > 1e-3 * top.max()
    spread = ((top - s.min(1)) / np.where(live, top, 1))[live]
    assert np.median(spread) > 1e3 * TWIN and np.median(spread) < 1e-4, np.median(spread)


def _settled_cells(res):
    """Cells whose amp / snr are float64 patches of the settle (not float32 values widened)."""
    snr = np.asarray(res[3])
    return (snr != snr.astype(np.float32).astype(np.float64)) & (snr > 0)


@pytest.mark.parametrize("cls,method,route", [(NearTiePlugin, "fft", "fft"), (NearTieMaskedPlugin, "fft", "direct"),
                                              (NearTieMaskedPlugin, "auto", None)])
def test_near_tie_plugin_exact_is_the_float64_argmax(gpu_ctx, noise_dem, oracle_plain, oracle_masked, cls, method, route):
    amp_st, snr_st = oracle_plain if cls is NearTiePlugin else oracle_masked
    g = grid(noise_dem, 1.0)
    m = sl.Matcher(g, ctx=gpu_ctx)
    try:
        t0 = time.perf_counter()
        r32 = np.stack(m.search(cls, 10.0, PLUGIN_AGES, PLUGIN_ANGLES, method=method, exact=False).result()).copy()
        t1 = time.perf_counter()
        res = np.stack(m.search(cls, 10.0, PLUGIN_AGES, PLUGIN_ANGLES, method=method, exact=True).result())
        t2 = time.perf_counter()
        st = dict(m.exact_stats)
    finally:
        gpu_ctx.clear_windows()
    n32, _ = _off_argmax(r32, snr_st, PLUGIN_AGES, PLUGIN_ANGLES)
    n64, bad = _off_argmax(res, snr_st, PLUGIN_AGES, PLUGIN_ANGLES)
    print("%s %s: %s route, float32 search %d cells off the float64 argmax, exact %d (of %d); exact_stats %s; "
          "wall %.3f s (exact=False %.3f s)" % (cls.__name__, method, m.method_used, n32, n64, bad.size, st, t2 - t1, t1 - t0))
    assert st.get("route") == "device" and "skipped" not in st, st
    if route is not None:
        assert m.method_used == route
    assert n32 > 0.01 * bad.size, n32                  # (by construction: float32 cannot order the ages)
    assert n64 == 0, (n64, np.argwhere(bad)[:5])
    assert st["changed_cells"] > 0
    assert np.isfinite(st["max_f32_err"]) and st["max_f32_err"] > 0
    # the settled cells carry the oracle's float64 amplitude and SNR of the template they hold
    sel = _settled_cells(res)
    assert sel.sum() > 0
    k = _template_index(res, PLUGIN_AGES, PLUGIN_ANGLES)[sel]
    ii, jj = np.nonzero(sel)
    a64, s64 = amp_st[k, ii, jj], snr_st[k, ii, jj]
    assert np.allclose(res[3][sel], s64, rtol=1e-12, atol=0), np.abs(res[3][sel] / s64 - 1).max()
    assert np.allclose(res[0][sel], a64, rtol=1e-12, atol=1e-14 * np.abs(amp_st).max()), np.abs(res[0][sel] - a64).max()


def test_near_tie_plugin_exact_is_deterministic(gpu_ctx, noise_dem):
    g = grid(noise_dem, 1.0)
    m = sl.Matcher(g, ctx=gpu_ctx)
    try:
        a = np.stack(m.search(NearTieMaskedPlugin, 10.0, PLUGIN_AGES, PLUGIN_ANGLES, exact=True).result()).copy()
        b = np.stack(m.search(NearTieMaskedPlugin, 10.0, PLUGIN_AGES, PLUGIN_ANGLES, exact=True).result())
    finally:
        gpu_ctx.clear_windows()
    assert a.tobytes() == b.tobytes()


def test_score_f64_on_window_templates(gpu_ctx, noise_dem, oracle_masked):
    """sc_score_cells_f64 / sc_score_pairs_f64 on uploaded windows: the oracle's float64 values, masks included."""
    amp_st, snr_st = oracle_masked
    ny, nx = noise_dem.shape
    t = NearTieMaskedPlugin(10.0, 1.0, PLUGIN_ANGLES[2], nx, ny, 1.0)
    lim, err = t.get_window_limits(), t.get_err_mask()
    cells = [(60, 70), (100, 101), (41, 31), (2, 50)]                    # two live cells, two in the limit mask
    cells += [tuple(int(v) for v in np.argwhere(err & ~lim)[0]), tuple(int(v) for v in np.argwhere(~err & ~lim)[7])]
    cells = np.array(cells, dtype=np.int32)
    assert lim[cells[2][0], cells[2][1]] and lim[cells[3][0], cells[3][1]] and err[cells[4][0], cells[4][1]]
    g = grid(noise_dem, 1.0)
    m = sl.Matcher(g, ctx=gpu_ctx)
    try:
        m.search(NearTieMaskedPlugin, 10.0, PLUGIN_AGES, PLUGIN_ANGLES, method="direct", exact=False)
        n_t = len(PLUGIN_AGES) * len(PLUGIN_ANGLES)
        amp, snr = gpu_ctx.score_cells_f64(cells, n_t)
        tsel = np.arange(len(cells), dtype=np.int32) * 3 % n_t
        amp_p, snr_p = gpu_ctx.score_pairs_f64(cells, tsel)
    finally:
        gpu_ctx.clear_windows()
    a_ref = amp_st[:, cells[:, 0], cells[:, 1]].T                       # (cells, templates)
    s_ref = snr_st[:, cells[:, 0], cells[:, 1]].T
    atol = 1e-14 * np.abs(amp_st).max()
    assert np.allclose(snr, s_ref, rtol=1e-12, atol=0), np.abs(snr - s_ref).max()
    assert np.allclose(amp, a_ref, rtol=1e-12, atol=atol)
    # the limit mask zeroes amplitude and SNR, the error mask (of the third orientation) the SNR of its templates
    n_a = len(PLUGIN_AGES)
    assert (snr[2:4] == 0).all() and (amp[2:4] == 0).all() and (snr[:2] > 0).all()
    assert (snr[4, 2 * n_a:3 * n_a] == 0).all() and (amp[4, 2 * n_a:3 * n_a] != 0).all()
    rows = np.arange(len(cells))
    assert np.allclose(snr_p, s_ref[rows, tsel], rtol=1e-12, atol=0)
    assert np.allclose(amp_p, a_ref[rows, tsel], rtol=1e-12, atol=atol)


def test_audit_retries_a_window_too_narrow(gpu_ctx, noise_dem, oracle_masked):
    """A near-tie window far below the float32 error: the audit trips, the search and the settle run once more with a
    window of at least the path's default, and the result is still the float64 argmax."""
    _, snr_st = oracle_masked
    g = grid(noise_dem, 1.0)
    m = sl.Matcher(g, ctx=gpu_ctx)
    m.EXACT_WINDOW_DIRECT = 1e-7
    m.EXACT_WINDOW = {k: 1e-7 for k in sl.Matcher.EXACT_WINDOW}
    try:
        res = np.stack(m.search(NearTieMaskedPlugin, 10.0, PLUGIN_AGES, PLUGIN_ANGLES, exact=True).result())
        st = dict(m.exact_stats)
    finally:
        gpu_ctx.clear_windows()
    print("retry: %s" % st)
    assert "retried" in st, st
    old, new = st["retried"]
    assert old == 1e-7 and new >= sl.Matcher.EXACT_WINDOW_DIRECT
    n64, bad = _off_argmax(res, snr_st, PLUGIN_AGES, PLUGIN_ANGLES)
    assert n64 == 0, (n64, np.argwhere(bad)[:5])


def test_audit_on_a_builtin_search(gpu_ctx):
    """Built-in classes report the audit and keep their windows: no retry."""
    z = np.load(golden("carrizo_crop.npy"))
    m = sl.Matcher(grid(z, 1.0), ctx=gpu_ctx)
    m.search(sl.Scarp, 100, _plan.age_grid(), _plan.angle_grid(-np.pi / 2, np.pi / 2)[::4], method="fft", exact=True)
    st = dict(m.exact_stats)
    win = st.get("window")
    print("carrizo crop, Scarp: %s (%s path, window %.1e)" % (st, m.method_used, win))
    assert st.get("route") == "device" and "retried" not in st and st["float64_cells"] > 0
    assert np.isfinite(st["max_f32_err"]) and 0 < st["max_f32_err"] < 0.5 * win


# ---- the reference's serial driver on a Shifted class -----------------------------------------------------------------
@pytest.fixture(scope="module")
def serial_case():
    c = np.load(golden("ref_serial.npz"))
    z = np.asarray(c["z"])
    ny, nx = z.shape
    de = float(c["de"])
    kw = dict(dx=int(c["sdx"]), dy=int(c["sdy"]))
    ages = _plan.age_grid()
    angles = _plan.angle_grid(float(c["ang_min"]), float(c["ang_max"]))
    scale = float(c["scale"])
    amp, snr = _stack(np.asarray(z, dtype=float), de, de,
                      lambda par, ang: WT.ShiftedLeftFacingUpperBreakScarp(scale, par, ang, nx, ny, de, **kw), ages, angles)
    return dict(z=z, de=de, kw=kw, ages=ages, angles=angles, scale=scale, gold=c["res"], amp=amp, snr=snr)


@pytest.mark.parametrize("method", ["auto", "direct"])
def test_serial_golden_shifted_exact(gpu_ctx, serial_case, method):
    c = serial_case
    m = sl.Matcher(grid(c["z"], c["de"]), ctx=gpu_ctx)
    try:
        t0 = time.perf_counter()
        m.search(WT.ShiftedLeftFacingUpperBreakScarp, c["scale"], c["ages"], c["angles"], method=method, exact=False,
                 **c["kw"]).result()
        t1 = time.perf_counter()
        res = m.search(WT.ShiftedLeftFacingUpperBreakScarp, c["scale"], c["ages"], c["angles"], method=method,
                       exact=True, **c["kw"]).result()
        t2 = time.perf_counter()
        st = dict(m.exact_stats)
        win = st.get("window")
    finally:
        gpu_ctx.clear_windows()
    gold = c["gold"]
    live = gold[3] > 0
    mine = _template_index(res, c["ages"], c["angles"])
    ref = _template_index(gold, c["ages"], c["angles"])
    same = mine == ref
    ii, jj = np.nonzero(live & ~same)
    s = c["snr"]
    twin = (mine[ii, jj] >= 0) & (np.abs(s[np.maximum(mine[ii, jj], 0), ii, jj] - s[ref[ii, jj], ii, jj])
                                  <= TWIN * s[ref[ii, jj], ii, jj])
    n_bad = int((~twin).sum())
    print("serial golden, Shifted, %s (%s path): %d live cells, %d with the reference's (age, angle), %d twins, %d off; "
          "exact_stats %s; wall %.3f s (exact=False %.3f s)"
          % (method, m.method_used, int(live.sum()), int((same & live).sum()), int(twin.sum()), n_bad, st, t2 - t1, t1 - t0))
    assert st.get("route") == "device" and "skipped" not in st, st
    assert n_bad == 0, list(zip(ii[~twin][:5], jj[~twin][:5]))
    # the audit: measured, and inside half the window the search flagged with
    assert win is not None and np.isfinite(st["max_f32_err"]) and st["max_f32_err"] < 0.5 * win, st
    assert "retried" not in st
