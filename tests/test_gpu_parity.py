"""Parity of the HIP paths with the oracle and the reference's golden vectors.

Every test calls through the C ABI (scarplet_amd._lib -> libscarplet_hip.so).

Stated tolerances (float32 device arithmetic vs the float64 reference):
  amp : |d| <= AMP_RTOL * |amp| + AMP_ATOL * max|amp|
  snr : |d| <= SNR_RTOL * snr  + SNR_ATOL * max(snr)
  argmax (age, angle): exact, except where the oracle's best and the chosen
  template's SNR differ by less than the tie window of the device path that
  ran (oracle.tie_window: 7e-4 FFT tiles, 1e-4 real space) - twice the largest
  SNR error measured on that path (near-tie policy, see oracle.check_fold and
  DESIGN.md "Parity").  Every fold test prints and asserts the fraction of
  cells that carry exactly the oracle's argmax (EXACT_MIN) and that its own
  measured SNR error is at most HALF the window (report()).
"""
import warnings

import numpy as np
import pytest

import scarplet_oracle as orc
import scarplet_amd as sl
from scarplet_amd import _plan, synthetic
from scarplet_amd import WindowedTemplate as WT
from conftest import golden, load_cases
from parity_report import report

pytestmark = pytest.mark.gpu

AMP_RTOL, AMP_ATOL = orc.PARITY["amp"]
SNR_RTOL, SNR_ATOL = orc.PARITY["snr"]
TIE_RTOL = orc.PARITY["tie_rtol"]      # twice the measured SNR error (oracle.PARITY)
EXACT_MIN = 0.99                       # surfaces WITHOUT a noise floor only: share of cells on the oracle's argmax


CLS = {"scarp": WT.Scarp, "ricker": WT.Ricker,
       "right_upper_break": WT.RightFacingUpperBreakScarp,
       "left_upper_break": WT.LeftFacingUpperBreakScarp}


def close_maps(amp, snr, o_amp, o_snr):
    ea = np.abs(amp - o_amp) <= AMP_RTOL * np.abs(o_amp) + AMP_ATOL * np.max(np.abs(o_amp)) + 1e-30
    es = np.abs(snr - o_snr) <= SNR_RTOL * np.abs(o_snr) + SNR_ATOL * np.max(np.abs(o_snr)) + 1e-30
    return ea.all() and es.all(), (float(np.max(np.abs(amp - o_amp))), float(np.max(np.abs(snr - o_snr))))


def grid(z, dx, dy=None):
    return sl.DEMGrid.from_array(z, float(dx), None if dy is None else float(dy))


# ------------------------------------------------------------------ K1
def test_curvature_reference_goldens(gpu_ctx):
    f = np.load(golden("ref_faultzone_curvature.npz"))
    for name, sl_y, sl_x in (("tl", slice(None, -1), slice(None, -1)), ("br", slice(1, None), slice(1, None))):
        z = f["z_" + name]
        m = sl.Matcher(grid(z, 2.0, 2.0), ctx=gpu_ctx)
        for deg, ang in zip((0, -90, -45, 45, 90), (0.0, -np.pi / 2, -np.pi / 4, np.pi / 4, np.pi / 2)):
            c = m.ctx.curvature(*_plan.curvature_coefficients(ang), z.shape)
            gold = f["gold_%s_%d" % (name, deg)]
            assert np.allclose(c[sl_y, sl_x], gold[sl_y, sl_x], rtol=1e-5, atol=1e-6 * np.max(np.abs(gold)))


def test_data_object_curvature_methods(gpu_ctx):
    """DEMGrid._calculate_directional_laplacian / _calculate_laplacian (dem.py:62-107): the
    methods the reference's own tests call (tests/test_dem.py:34,42), float64 out, against the
    reference's golden crops cell for cell; NaN cells zeroed before the stencils and NaN in the
    result (dem.py:85-86, 105), the grid keeping the zeros like the reference's."""
    f = np.load(golden("ref_faultzone_curvature.npz"))
    for name, sl_y, sl_x in (("tl", slice(None, -1), slice(None, -1)), ("br", slice(1, None), slice(1, None))):
        g = grid(f["z_" + name], 2.0, 2.0)
        for deg, ang in zip((0, -90, -45, 45, 90), (0.0, -np.pi / 2, -np.pi / 4, np.pi / 4, np.pi / 2)):
            c = g._calculate_directional_laplacian(ang)
            assert c.dtype == np.float64
            gold = f["gold_%s_%d" % (name, deg)]
            assert np.array_equal(c[sl_y, sl_x], gold[sl_y, sl_x]), (name, deg, np.abs(c - gold)[sl_y, sl_x].max())
        assert np.array_equal(g._calculate_laplacian(), g._calculate_directional_laplacian(0))
    rng = np.random.default_rng(5)
    z = rng.standard_normal((37, 53)).cumsum(1)
    z[4, 7] = z[20, 30:33] = np.nan
    g = grid(z.copy(), 1.5, 2.5)
    got = g._calculate_directional_laplacian(0.3)
    z0 = np.where(np.isnan(z), 0.0, z)
    want = orc.directional_curvature(z0, 1.5, 2.5, 0.3)
    want[np.isnan(z)] = np.nan
    assert np.array_equal(got, want, equal_nan=True)
    assert not np.isnan(g._griddata).any() and np.array_equal(g._griddata, z0)


# ------------------------------------------------------------------ K2..K4
@pytest.mark.parametrize("method", ["direct", "fft"])
def test_match_template_reference_outputs(gpu_ctx, method):
    """amp / snr maps and the per-template scalars n, sum(W^2) against values
    captured from the reference's match_template (core.py:297-377)."""
    for c in load_cases("ref_match_template.npz"):
        g = grid(c["z"], c["dx"], c["dy"])
        m = sl.Matcher(g, ctx=gpu_ctx)
        amp, snr = m.match_template(CLS[str(c["kind"])], float(c["scale"]), float(c["age"]),
                                    float(c["ang"]), method=method)
        n, ts = m.ctx.template_sums(1)
        assert abs(n[0] - float(c["n"])) < 1e-6, "support size differs from the reference"
        assert np.isclose(ts[0], float(c["ts"]), rtol=1e-12)
        ok, err = close_maps(amp, snr, c["amp"], c["snr"])
        assert ok, (str(c["kind"]), method, err)


@pytest.mark.parametrize("method", ["direct", "fft"])
@pytest.mark.parametrize("shape", [(64, 64), (61, 75), (96, 63), (65, 65), (200, 130)])
def test_match_template_even_odd_sizes(gpu_ctx, method, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    z = (np.cumsum(rng.standard_normal(shape), 1) * 0.03 + rng.standard_normal(shape) * 0.04).astype(np.float32)
    for de, scale, age, ang in [(1.0, 9, 4.0, 0.7), (2.0, 22, 20.0, -1.3), (1.0, 6, 1.0, 0.0)]:
        m = sl.Matcher(grid(z, de), ctx=gpu_ctx)
        amp, snr = m.match_template(WT.Scarp, scale, age, ang, method=method)
        o_amp, _, _, o_snr = orc.match_template(z, de, de, orc.SCARP, scale, age, ang)
        ok, err = close_maps(amp, snr, o_amp, o_snr)
        assert ok, (shape, de, scale, age, ang, err)


def test_fft_tiling_is_invisible(gpu_ctx):
    """Overlap-save with different tile sizes, and the real-space path, give
    the same maps (within float32 noise) on a DEM larger than one tile."""
    g = synthetic.synthetic_scarp(700, seed=3)
    z = g._griddata
    m = sl.Matcher(g, ctx=gpu_ctx)
    o_amp, _, _, o_snr = orc.match_template(z, 1.0, 1.0, orc.SCARP, 30, 50.0, 0.9)
    outs = {}
    for tmax in (256, 512, 1024):
        arr, bbox, area = m.describe(WT.Scarp, 30, [50.0], [0.9])
        p = _plan.Plan(m.ny, m.nx, m.core, bbox, whole=True, method=_plan.METHOD_FFT, t_max=tmax)
        sp = sl._lib.sc_plan(method=1, Ty=p.Ty, Tx=p.Tx, Vy=p.Vy, Vx=p.Vx, nty=p.nty, ntx=p.ntx,
                             circ_y=int(p.circ_y), circ_x=int(p.circ_x), Py=p.Py, Qx=p.Qx, group=1)
        assert p.nty * p.ntx > 1
        outs[tmax] = m.ctx.match_template(arr[0], sp)
        ok, err = close_maps(outs[tmax][0], outs[tmax][1], o_amp, o_snr)
        assert ok, (tmax, err)
    amp_d, snr_d = m.match_template(WT.Scarp, 30, 50.0, 0.9, method="direct")
    assert close_maps(amp_d, snr_d, o_amp, o_snr)[0]


# ------------------------------------------------------------------ K5 + drivers
def fold_check(res, z, dx, dy, kind, scale, params, angles, method="fft"):
    a_st, s_st = orc.snr_stack(z, dx, dy, kind, scale, params, angles)
    T = len(params) * len(angles)
    ny, nx = z.shape
    ages = np.repeat(np.asarray(params, float), len(angles))
    angs = np.tile(np.asarray(angles, float), len(params))
    return orc.check_fold(res, a_st.reshape(T, ny, nx), s_st.reshape(T, ny, nx), ages, angs,
                          tie_rtol=orc.tie_window(method, kind), amp_tol=(AMP_RTOL, AMP_ATOL * np.max(np.abs(a_st))),
                          snr_tol=(orc.snr_tolerance(kind)[0], orc.snr_tolerance(kind)[1] * np.max(s_st)))


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_fold_against_oracle_stack(gpu_ctx, method):
    rng = np.random.default_rng(21)
    z = (np.cumsum(np.cumsum(rng.standard_normal((96, 90)), 0), 1) * 0.01
         + rng.standard_normal((96, 90)) * 0.05).astype(np.float32)
    params = [1.0, 3.16, 10.0, 31.6]
    angles = _plan.angle_grid(-0.6, 0.6)
    m = sl.Matcher(grid(z, 1.0), ctx=gpu_ctx)
    res = m.search(WT.Scarp, 10, params, angles, method=method).result()
    chk = fold_check(res, z, 1.0, 1.0, orc.SCARP, 10, params, angles, method)
    report("oracle stack 96x90 %s" % method, chk, method)
    assert chk["n_bad"] == 0, chk
    assert chk["exact_frac"] >= EXACT_MIN, chk


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_fold_channel_even_template(gpu_ctx, method):
    """Ricker is even in xr: -pi/2 and +pi/2 tie exactly; the near-tie policy
    must classify those cells, everything else must match strictly."""
    rng = np.random.default_rng(22)
    z = (np.cumsum(rng.standard_normal((80, 96)), 0) * 0.04 + rng.standard_normal((80, 96)) * 0.03).astype(np.float32)
    params = [0.1, 0.2]
    angles = _plan.angle_grid()[::6]
    m = sl.Matcher(grid(z, 1.0, -1.0), ctx=gpu_ctx)
    res = m.search(WT.Channel, 6, params, angles, method=method).result()
    chk = fold_check(res, z, 1.0, -1.0, orc.RICKER, 6, params, angles, method)
    report("channel (even template: -90/+90 tie) %s" % method, chk, method)
    assert chk["n_bad"] == 0, chk
    # (-pi/2 and +pi/2 are the same template: check_fold counts either as the argmax)
    assert chk["exact_frac"] >= EXACT_MIN, chk


def test_small_searches_reference(gpu_ctx):
    """sl.match against outputs captured from the reference's sl.match."""
    for c in load_cases("ref_match_small.npz"):
        kw = dict(zip([str(k) for k in c["keys"]], [float(v) for v in c["vals"]]))
        kind = str(c["kind"])
        g = grid(c["z"], c["dx"], c["dy"])
        res = sl.match(g, CLS[kind], **kw)
        angles = _plan.angle_grid(kw["ang_min"], kw["ang_max"])
        params = [kw["age"]] if "age" in kw else list(_plan.age_grid())
        chk = fold_check(res, c["z"], float(c["dx"]), float(c["dy"]), kind, kw["scale"], params, angles)
        report("reference sl.match capture (%s)" % kind, chk)
        assert chk["n_bad"] == 0, (kind, chk)
        if kind != "ricker":
            # (ages: numpy's 10**x differs by an ulp between the numpy that wrote the fixture and this one)
            same = np.isclose(res[1], c["res"][1], rtol=1e-9) & (np.asarray(res[2]) == c["res"][2])
            print("     same (age, angle) as the reference's output: %.4f" % same.mean())
            assert same.mean() >= EXACT_MIN, float(same.mean())
        # (sl.match is exact by default, and report() above holds it to n_inexact == 0 against the same oracle stack: a
        #  cell whose (age, angle) differs from the capture - Ricker's end twins included - is an oracle co-maximum.  The
        #  float32 mode is exact on these small searches as well, so no float32 count can show teeth here.)


def _fold_twin(ang):
    """the orientation plane with the grid's end twins as one (+pi/2 is -pi/2 for the symmetric built-ins)"""
    a = np.array(ang, dtype=float)
    a[np.abs(a - np.pi / 2) < 1e-12] = -np.pi / 2
    return a


def _probe_golden(name, res, res32, gold, z, kind, scale, ages, angles, pool, n_agree=24):
    """The exact result's cells against the oracle's float64 argmax over the WHOLE template grid: every live cell whose
    (age, angle) differs from the reference's capture ``gold`` (the grid's end twins as one), ``n_agree`` random agreeing
    cells, and the cells where the float32 search ``res32`` names another template than ``res``.  A cell is off when the
    template it carries scores below (1 - 1e-9) of the cell's largest float64 SNR (check_fold's rule).  Returns
    (cells of res off the argmax, cells of res32 off it among those where it differs from res, probes)."""
    par, ang = np.repeat(np.asarray(ages, float), len(angles)), np.tile(np.asarray(angles, float), len(ages))

    def same(a, b):
        return np.isclose(a[1], b[1], rtol=1e-9) & (_fold_twin(a[2]) == _fold_twin(b[2]))
    live = (np.asarray(res[3]) > 0) | (np.asarray(gold[3]) > 0)
    differ = live & ~same(res, gold)
    differ32 = live & ~same(res, res32)
    rng = np.random.default_rng(12)
    agree = np.argwhere(live & ~differ)
    agree = agree[rng.permutation(len(agree))[:n_agree]]
    cells = np.unique(np.concatenate([np.argwhere(differ), agree, np.argwhere(differ32)]), axis=0)
    S = orc.snr_at_cells(z, 1.0, 1.0, kind, scale, ages, angles, cells, pool)          # (T, n_cells)
    smax = S.max(axis=0)
    floor = SNR_ATOL * float(np.max(res[3]))          # (below the absolute SNR tolerance: nothing to decide)

    def off_of(r):
        off = np.zeros(len(cells), bool)
        for k, (i, j) in enumerate(cells):
            t = np.flatnonzero(np.isclose(par, r[1][i, j], rtol=1e-9) & (ang == r[2][i, j]))
            off[k] = smax[k] > floor and (not len(t) or S[t[0], k] < smax[k] * (1.0 - 1e-9))
        return off
    off, off32 = off_of(res), off_of(res32)
    sel32 = np.array([bool(differ32[i, j]) for (i, j) in cells], bool)
    print("%s: %d live cells differ from the capture, %d agreeing probed; %d probes x %d templates: %d cells of the "
          "exact result off the oracle's argmax; the float32 search differs from it in %d cells, %d of them off the argmax"
          % (name, int(differ.sum()), len(agree), len(cells), len(par), int(off.sum()), int(differ32.sum()),
             int((off32 & sel32).sum())))
    return int(off.sum()), int((off32 & sel32).sum()), int(differ32.sum())


def golden_check(res, gold, tie_rtol=orc.tie_window("fft", orc.SCARP)):
    """Against a reference golden without the per-template stack: cells whose
    (age, angle) equal the golden's must match in amp/snr; any other cell must
    be a near-tie, i.e. reach the golden's (maximal) SNR within the tie window of
    the template family (the reference's goldens are Scarp searches: 1e-4)."""
    TIE_RTOL = tie_rtol
    amp, age, ang, snr = [np.asarray(a) for a in res]
    g_amp, g_age, g_ang, g_snr = gold
    same = np.isclose(age, g_age, rtol=1e-9) & (ang == g_ang)
    tol_a = AMP_RTOL * np.abs(g_amp) + AMP_ATOL * np.max(np.abs(g_amp)) + 1e-30
    tol_s = SNR_RTOL * g_snr + SNR_ATOL * np.max(g_snr) + 1e-30
    ok_same = same & (np.abs(amp - g_amp) <= tol_a) & (np.abs(snr - g_snr) <= tol_s)
    near = ~same & (snr >= g_snr * (1 - TIE_RTOL)) & (snr <= g_snr * (1 + TIE_RTOL) + tol_s) & (g_snr > 0)
    return ok_same, near


def test_synthetic_single_age_golden(gpu_ctx, oracle_pool):
    """scarplet/tests/test_core.py:47-64 (synthetic_match2.npy)."""
    z = np.load(golden("ref_synthetic_dem.npy"))
    gold = np.load(golden("ref_synthetic_match2.npz"))["res"]
    res = sl.match(grid(z, 1.0), sl.Scarp, scale=100, age=10, ang_max=np.pi / 2, ang_min=-np.pi / 2)
    assert res.shape == (4, 200, 200) and res.dtype == np.float64
    ok_same, near = golden_check(res, gold)
    print("golden synthetic_match2: same (age, angle) and values %.4f, near-tie %.4f" % (ok_same.mean(), near.mean()))
    assert (ok_same | near).all()
    assert ok_same.mean() >= EXACT_MIN
    # the default sl.match is exact: counted against the oracle over all 181 templates, not as a share
    res32 = sl.match(grid(z, 1.0), sl.Scarp, scale=100, age=10, ang_max=np.pi / 2, ang_min=-np.pi / 2, exact=False)
    n_off, n_off32, n_diff32 = _probe_golden("golden synthetic_match2", res, res32, gold, np.asarray(z, float), orc.SCARP,
                                             100.0, [10.0], _plan.angle_grid(), oracle_pool)
    assert n_off == 0, n_off
    assert n_diff32 == 0 or n_off32 >= 1, (n_diff32, n_off32)     # (where float32 differs, it is the one off the argmax)


def test_synthetic_full_grid_golden(gpu_ctx, oracle_pool):
    """scarplet/tests/test_core.py:28-45 (synthetic_match1.npy): the only
    end-to-end pin of the 35 x 181 search in the reference."""
    z = np.load(golden("ref_synthetic_dem.npy"))
    gold = np.load(golden("ref_synthetic_match1.npz"))["res"]
    res = sl.match(grid(z, 1.0), sl.Scarp, scale=100, ang_max=np.pi / 2, ang_min=-np.pi / 2)
    assert isinstance(res, tuple) and len(res) == 4
    ok_same, near = golden_check(res, gold)
    bad = ~(ok_same | near)
    print("golden synthetic_match1: same (age, angle) and values %.4f, near-tie %.4f" % (ok_same.mean(), near.mean()))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
    assert ok_same.mean() >= EXACT_MIN, float(ok_same.mean())
    # the default sl.match is exact: counted against the oracle over all 6335 templates, not as a share
    res32 = sl.match(grid(z, 1.0), sl.Scarp, scale=100, ang_max=np.pi / 2, ang_min=-np.pi / 2, exact=False)
    n_off, n_off32, n_diff32 = _probe_golden("golden synthetic_match1", res, res32, gold, np.asarray(z, float), orc.SCARP,
                                             100.0, _plan.age_grid(), _plan.angle_grid(), oracle_pool)
    assert n_off == 0, n_off
    assert n_diff32 == 0 or n_off32 >= 1, (n_diff32, n_off32)     # (where float32 differs, it is the one off the argmax)


def test_noise_free_surfaces_resolution_floor(gpu_ctx):
    """Float32 resolution of the FFT path, stated and tested.  On surfaces without a noise floor
    (synthetic erf scarps stored as float32, a ramp added: the ground away from the feature
    carries quantisation noise only) a float32 FFT convolution cannot resolve residuals T3 - T1
    that lie 1e-7 below the tile's energy; the device clamps them (sc_epi_floor) and reports an
    SNR that is off by about (float32 resolution of the residual) / (residual).
    oracle.resolution_floor() evaluates that ratio per (template, cell) as an extra relative
    tolerance ("slack", 32 f / r); check_fold applies it to the values and to the tie window.
    The real-space path has no such limit: it must match everywhere with the plain tolerances.  (The floor constant kappa = 4 was calibrated on the reference's
    synthetic.tif; these are three further surfaces: de = 2 / scale = 20, a channel under Ricker
    templates, and a scarp on a ramp crossing several tiles.)"""
    from scipy.special import erf
    cases = []
    y, x = np.mgrid[-100:100, -100:100].astype(float) * 2.0
    cases.append((-erf((-x * np.sin(0.6) + y * np.cos(0.6)) / (2 * np.sqrt(25.0))), 2.0, 2.0, WT.Scarp, orc.SCARP,
                  20, [5.0, 25.0, 100.0], _plan.angle_grid()[::15], _plan.T_MAX))
    y, x = np.mgrid[-128:128, -128:128].astype(float)
    d = -x * np.sin(-0.4) + y * np.cos(-0.4)
    cases.append((-np.exp(-(d / 6.0) ** 2), 1.0, -1.0, WT.Channel, orc.RICKER, 10, [0.05, 0.1],
                  _plan.angle_grid()[::12], _plan.T_MAX))
    y, x = np.mgrid[-300:300, -330:330].astype(float)
    cases.append((-erf((-x * np.sin(1.1) + y * np.cos(1.1)) / (2 * np.sqrt(10.0))) + 0.01 * x, 1.0, 1.0,
                  WT.Scarp, orc.SCARP, 40, [3.0, 10.0, 30.0], _plan.angle_grid()[5::30], 256))
    failures = []
    for (z, dx, dy, cls, kind, scale, params, angles, tmax) in cases:
        z = z.astype(np.float32)
        ny, nx = z.shape
        T = len(params) * len(angles)
        A, S, K = orc.resolution_floor(z, dx, dy, kind, scale, params, angles, workers=4)
        A, S, K = A.reshape(T, ny, nx), S.reshape(T, ny, nx), K.reshape(T, ny, nx)
        ages_t, angs_t = np.repeat(params, len(angles)), np.tile(angles, len(params))
        tol = dict(tie_rtol=TIE_RTOL, amp_tol=(AMP_RTOL, AMP_ATOL * np.abs(A).max()),
                   snr_tol=(orc.snr_tolerance(kind)[0], orc.snr_tolerance(kind)[1] * S.max()))
        m = sl.Matcher(grid(z, dx, dy), ctx=gpu_ctx)
        arr, bbox, area = m.describe(cls, scale, np.asarray(params, float), np.asarray(angles, float))
        p = _plan.Plan(m.ny, m.nx, m.core, bbox, whole=True, method=_plan.METHOD_FFT, t_max=tmax)
        sp = sl._lib.sc_plan(method=1, Ty=p.Ty, Tx=p.Tx, Vy=p.Vy, Vx=p.Vx, nty=p.nty, ntx=p.ntx,
                             circ_y=int(p.circ_y), circ_x=int(p.circ_x), Py=p.Py, Qx=p.Qx, group=len(params))
        m.ctx.reset_best()
        m.ctx.match(arr, sp)
        res = m.ctx.get_result(ages_t, angs_t)
        chk = orc.check_fold(res, A, S, ages_t, angs_t, slack=K, **tol)
        name = "noise-free %s %dx%d de=%g tiles %dx%d" % (kind, ny, nx, dx, p.nty, p.ntx)
        report(name + " fft", chk, window=float("inf"), noise_floor=False)       # outside the window policy: the slack states it per cell
        print("     (template, cell) pairs with slack > 1e-3: %.3f; cells accepted through the slack: %d, below the "
              "absolute tolerance: %d" % ((K > 1e-3).mean(), chk["n_slack"], chk["n_below"]))
        # what the FFT path delivers on such a surface: every cell inside its stated resolution
        # (n_bad == 0) and at least nine cells in ten still on the oracle's own argmax
        # (measured 0.902 / 0.987 / 0.878 of the DECIDABLE cells - those below the absolute SNR tolerance on both
        #  sides, a third to a half of such a surface, are no longer counted as exact); method="auto" does not
        #  take this path here
        # (test_auto_takes_the_exact_path_without_a_noise_floor)
        if chk["n_bad"] or chk["exact_frac"] < 0.85:
            failures.append((name, "fft", chk["n_bad"], chk["exact_frac"]))
            for (i, j) in np.argwhere(~chk["ok"])[:6]:
                t_dev = np.nonzero((ages_t == res[1][i, j]) & (angs_t == res[2][i, j]))[0]
                t_max = int(np.argmax(S[:, i, j]))
                print("     bad cell (%d,%d): device amp %.6g snr %.6g template %s | oracle at it: amp %s snr %s slack %s | "
                      "oracle max: t=%d snr %.6g slack %.3g amp %.6g" % (
                          i, j, res[0][i, j], res[3][i, j], t_dev, A[t_dev, i, j], S[t_dev, i, j], K[t_dev, i, j],
                          t_max, S[t_max, i, j], K[t_max, i, j], A[t_max, i, j]))
        # the real-space path sums locally: no resolution limit, plain check
        res_d = m.search(cls, scale, params, angles, method="direct").result()
        chk_d = orc.check_fold(res_d, A, S, ages_t, angs_t, **tol)
        report(name + " direct", chk_d, window=TIE_RTOL, noise_floor=False)
        # exact but for ties below float32's own resolution: measured 0.9887 / 1.0 / 1.0, the cells off the argmax
        # hold two templates 1.4e-5 apart in the oracle's float64 SNRs (the real-space path's measured error: 7e-5)
        if chk_d["n_bad"] or chk_d["exact_frac"] < 0.98 or chk_d["inexact_gap"] > orc.tie_window("direct"):
            failures.append((name, "direct", chk_d["n_bad"], chk_d["exact_frac"], chk_d["inexact_gap"]))
    assert not failures, failures


def test_match_with_the_reference_fold(gpu_ctx):
    """sl.match(..., fold="reference"): the literal two-level fold (core.py:180-195, 288-292)
    with tie -> zero (core.py:230-240) over per-template device maps, against the oracle's
    literal fold (oracle.match)."""
    rng = np.random.default_rng(33)
    z = (np.cumsum(rng.standard_normal((72, 64)), 1) * 0.05 + rng.standard_normal((72, 64)) * 0.04).astype(np.float32)
    g = grid(z, 1.0)
    ages = [2.0, 8.0, 32.0]
    want = orc.match(z, 1.0, 1.0, orc.SCARP, ages=ages, scale=8, ang_min=-0.3, ang_max=0.3)
    got = sl.match(g, sl.Scarp, scale=8, ages=ages, ang_min=-0.3, ang_max=0.3, fold="reference")
    assert isinstance(got, tuple) and len(got) == 4 and got[0].shape == z.shape
    same = (got[1] == want[1]) & (got[2] == want[2])
    print("     reference fold, 3 ages x 35 orientations: same (age, angle) as the oracle's literal fold %.4f" % same.mean())
    assert same.mean() >= 0.99
    ok, err = close_maps(got[0][same], got[3][same], want[0][same], want[3][same])
    assert ok, err
    one = sl.match(g, sl.Scarp, scale=8, age=8.0, ang_min=-0.3, ang_max=0.3, fold="reference")
    ref1 = orc.match(z, 1.0, 1.0, orc.SCARP, scale=8, age=8.0, ang_min=-0.3, ang_max=0.3)
    assert one.shape == (4,) + z.shape and ((one[2] == ref1[2]).mean() >= 0.99)
    # the literal rule on an exact tie: Ricker is even in xr, -pi/2 and +pi/2 are ONE template -
    # bit-identical float32 maps, the record of a cell they share the maximum of is zeroed
    zc = (np.cumsum(rng.standard_normal((64, 64)), 0) * 0.04).astype(np.float32)
    r = sl.match(grid(zc, 1.0, -1.0), sl.Channel, scale=6., age=0.2, fold="reference")
    f = sl.match(grid(zc, 1.0, -1.0), sl.Channel, scale=6., age=0.2)
    tied = np.abs(f[2]) == np.pi / 2                     # the fused fold keeps the incumbent there
    assert tied.any() and (r[3][tied] == 0).all() and (r[0][tied] == 0).all()


def test_auto_takes_the_exact_path_without_a_noise_floor(gpu_ctx):
    """method="auto": on a synthetic surface without a noise floor the device's own resolution
    statistic (sc_get_resolution_stats: wins whose residual lies near the float32 floor of the
    transforms) sends the search to the real-space path - the result carries the oracle's argmax
    like the explicit direct search; on a DEM with a noise floor the statistic is ~0 and the
    FFT result stands."""
    from scipy.special import erf
    y, x = np.mgrid[-300:300, -330:330].astype(float)
    z = (-erf((-x * np.sin(1.1) + y * np.cos(1.1)) / (2 * np.sqrt(10.0))) + 0.01 * x).astype(np.float32)
    params, angles = [3.0, 10.0, 30.0], _plan.angle_grid()[5::30]
    m = sl.Matcher(grid(z, 1.0), ctx=gpu_ctx)
    with pytest.warns(UserWarning, match="exact real-space path"):
        res = m.search(WT.Scarp, 40, params, angles, method="auto").result()
    assert m.method_used == "direct" and m.unresolved_frac > m.UNRESOLVED_MAX
    chk = fold_check(res, z, 1.0, 1.0, orc.SCARP, 40, params, angles, "fft")
    report("auto on a noise-free scarp 600x660 (unresolved %.3f -> direct)" % m.unresolved_frac, chk, window=TIE_RTOL,
           noise_floor=False)
    assert chk["n_bad"] == 0 and chk["exact_frac"] >= EXACT_MIN, chk
    # a DEM with a noise floor: nothing to fall back from
    g = synthetic.synthetic_scarp(600, seed=4)
    m = sl.Matcher(g, ctx=gpu_ctx)
    m.search(WT.Scarp, 20, params, angles, method="fft")
    wins, near = m.ctx.resolution_stats()
    print("     noisy 600x600: %d wins, %d near the floor" % (wins, near))
    assert wins > 0 and near <= 1e-4 * wins


# ------------------------------------------------------------------ plugin API
def test_generic_plugin_goes_through_the_window_path(gpu_ctx):
    """A user subclass with its own template() (docs/source/new_template.rst
    pattern) is evaluated on the host and uploaded."""
    class Notch(WT.Scarp):
        def _device_descriptor(self):
            return None                     # force the generic path

        def template(self):
            W = super().template()
            W[::3, :] = 0.0                 # not expressible analytically
            return W

    rng = np.random.default_rng(5)
    z = rng.standard_normal((72, 80)).cumsum(1).astype(np.float32) * 0.05
    g = grid(z, 1.0)
    for method in ("direct", "fft"):
        amp, _, _, snr = sl.match_template(g, Notch, 10, 8.0, 0.5, method=method)
        t = Notch(10, 8.0, 0.5, 80, 72, 1.0)
        curv = orc.directional_curvature(z, 1.0, 1.0, 0.5)
        o_amp, o_snr = orc.match_arrays(curv, t.template(), t.get_window_limits())
        assert close_maps(amp, snr, o_amp, o_snr)[0]


def test_generic_windows_with_holes_and_long_runs(gpu_ctx):
    """Uploaded windows exercise every row form of the real-space kernel: rows with holes
    (every other column zeroed: taps accumulate one by one), long rows without holes (the T3 sum
    shared between adjacent outputs, run ends at every offset within a group of four) and rows
    that start and end anywhere - against the oracle, both device paths."""
    class Holes(WT.Scarp):
        def _device_descriptor(self):
            return None

        def template(self):
            W = super().template()
            W[:, ::2] = 0.0
            return W

    class Ragged(WT.Scarp):                       # a wide window whose rows start / end at every offset
        def _device_descriptor(self):
            return None

        def template(self):
            W = np.zeros((self.ny, self.nx))
            cy, cx = self.ny // 2, self.nx // 2
            for r in range(-9, 10):
                lo, hi = cx - 20 - (r % 7), cx + 18 + (r * r) % 11
                W[cy + r, lo:hi] = np.cos(np.arange(hi - lo) * 0.3 + r) + 0.2
            return W

    rng = np.random.default_rng(15)
    z = (rng.standard_normal((90, 140)).cumsum(1) * 0.05 + rng.standard_normal((90, 140)) * 0.02).astype(np.float32)
    g = grid(z, 1.0)
    for cls in (Holes, Ragged):
        t = cls(12, 30.0, 0.4, 140, 90, 1.0)
        curv = orc.directional_curvature(z, 1.0, 1.0, 0.4)
        o_amp, o_snr = orc.match_arrays(curv, t.template(), t.get_window_limits())
        for method in ("direct", "fft"):
            amp, _, _, snr = sl.match_template(g, cls, 12, 30.0, 0.4, method=method)
            ok, err = close_maps(amp, snr, o_amp, o_snr)
            assert ok, (cls.__name__, method, err)


def test_upper_break_err_masks(gpu_ctx):
    rng = np.random.default_rng(6)
    z = rng.standard_normal((70, 66)).cumsum(0).astype(np.float32) * 0.05
    for cls, kind in ((WT.RightFacingUpperBreakScarp, orc.RIGHT_UPPER), (WT.LeftFacingUpperBreakScarp, orc.LEFT_UPPER)):
        for method in ("direct", "fft"):
            amp, _, _, snr = sl.match_template(grid(z, 1.0), cls, 10, 6.0, -0.4, method=method)
            o_amp, _, _, o_snr = orc.match_template(z, 1.0, 1.0, kind, 10, 6.0, -0.4)
            assert close_maps(amp, snr, o_amp, o_snr)[0]
            assert (snr[o_snr == 0] == 0).all()


def test_shifted_templates_reference_outputs(gpu_ctx):
    """Shifted UpperBreak templates (WindowedTemplate.py:307-431) through the generic
    window path, against amp / snr captured from the reference's match_template."""
    from test_templates import SHIFTED
    for c in load_cases("ref_shifted.npz"):
        g = grid(c["z"], float(c["de"]))
        for method in ("direct", "fft"):
            amp, _, _, snr = sl.match_template(g, SHIFTED[str(c["name"])], float(c["scale"]), float(c["age"]),
                                               float(c["ang"]), dx=int(c["sdx"]), dy=int(c["sdy"]), method=method)
            ok, err = close_maps(amp, snr, c["amp"], c["snr"])
            assert ok, (str(c["name"]), method, err)
            assert (snr[c["snr"] == 0] == 0).all()


def test_serial_driver_forwards_kwargs(gpu_ctx):
    """calculate_best_fit_parameters_serial is the one route to the Shifted templates
    (core.py:65-136 forwards **kwargs): all four planes against what the REFERENCE's own driver
    returned for the same call (tests/golden/ref_serial.npz, captured by oracle/gen_golden.py
    from the unmodified reference: 48 x 52 DEM, ShiftedLeftFacingUpperBreakScarp, dx=2, dy=1,
    35 ages x 6 orientations, angle-outer / age-inner flat fold)."""
    c = np.load(golden("ref_serial.npz"))
    z, gold = c["z"], c["res"]
    kw = dict(ang_max=float(c["ang_max"]), ang_min=float(c["ang_min"]), dx=int(c["sdx"]), dy=int(c["sdy"]))
    for method in ("direct", "fft"):
        res = sl.calculate_best_fit_parameters_serial(
            grid(z, float(c["de"])), WT.ShiftedLeftFacingUpperBreakScarp, float(c["scale"]), method=method, **kw)
        assert len(res) == 4 and res[0].shape == z.shape
        ok_same, near = golden_check(res, gold)
        zero = (gold[3] == 0) & (np.asarray(res[3]) == 0)       # cells every template masks (limits, error half-plane)
        bad = ~(ok_same | near | zero)
        print("serial driver capture (%s): same (age, angle) and values %.4f, near-tie %.4f, masked %.4f"
              % (method, ok_same.mean(), near.mean(), zero.mean()))
        assert not bad.any(), (method, int(bad.sum()), np.argwhere(bad)[:5])
        # the age and angle planes themselves: the reference's values in (almost) every cell
        live = gold[3] > 0
        same = np.isclose(res[1], gold[1], rtol=1e-9) & (np.asarray(res[2]) == gold[2])
        assert same[live].mean() >= EXACT_MIN, (method, float(same[live].mean()))
        assert set(np.unique(np.asarray(res[2])[live])) <= set(np.unique(gold[2])), method


def test_compare_is_the_reference_fold(gpu_ctx):
    f = np.load(golden("ref_fold.npz"))
    res = sl.compare(((f["amps"][i], f["ages"][i], f["angs"][i], f["snrs"][i])
                      for i in range(len(f["ages"]))), 2, 2)
    assert np.array_equal(np.stack(res), f["res"], equal_nan=True)
    rng = np.random.default_rng(1)
    rs = [(rng.standard_normal((33, 47)), float(k), 0.1 * k, np.abs(rng.standard_normal((33, 47)))) for k in range(7)]
    rs[3][3][5, 5] = rs[2][3][5, 5]               # an exact tie zeroes the record
    mine = sl.compare(iter(rs), 33, 47)
    ref = orc.compare(iter(rs), 33, 47)
    for a, b in zip(mine, ref):
        assert np.array_equal(a, b)


def test_compare_folds_plane_valued_results_like_match(gpu_ctx):
    """match() feeds compare() the (4, ny, nx) arrays of
    calculate_best_fit_parameters (core.py:288-292): age and angle are per-cell
    planes there, and docs/examples/multiprocessing_example.ipynb calls
    sl.compare([best, results], nx, ny) the same way."""
    rng = np.random.default_rng(2)
    ny, nx = 21, 34
    rs = []
    for k in range(5):
        amp, snr = rng.standard_normal((ny, nx)), np.abs(rng.standard_normal((ny, nx)))
        age = np.where(snr > 0.5, 10.0 ** k, 0.0)                # planes, zeros where nothing won
        ang = rng.choice(np.linspace(-1.5, 1.5, 7), size=(ny, nx))
        rs.append(np.stack([amp, age, ang, snr]))                # (4, ny, nx) arrays
    rs[3][3][4, 4] = rs[1][3][4, 4]
    rs.insert(2, (rng.standard_normal((ny, nx)), 3.0, 0.25, np.abs(rng.standard_normal((ny, nx)))))  # scalars mixed in
    mine = sl.compare(iter(rs), ny, nx)
    ref = orc.compare(iter(rs), ny, nx)
    for a, b in zip(mine, ref):
        assert np.array_equal(a, b)


def test_second_search_with_another_grid_keeps_its_winners(gpu_ctx):
    """Matcher.search(reset=False) folds a second parameter grid into the same
    record: cells won by the first search must still decode to ITS (age, angle)."""
    rng = np.random.default_rng(31)
    z = (np.cumsum(rng.standard_normal((80, 84)), 1) * 0.05 + rng.standard_normal((80, 84)) * 0.03).astype(np.float32)
    p1, a1 = [2.0, 20.0], np.array([-0.5, 0.1])
    p2, a2 = [5.0, 8.0, 50.0], np.array([0.7, -1.1, 1.3])
    m = sl.Matcher(grid(z, 1.0), ctx=gpu_ctx)
    m.search(WT.Scarp, 10, p1, a1, method="fft")
    m.search(WT.Scarp, 10, p2, a2, method="fft", reset=False)
    res = m.result()
    a_1, s_1 = orc.snr_stack(z, 1.0, 1.0, orc.SCARP, 10, p1, a1)
    a_2, s_2 = orc.snr_stack(z, 1.0, 1.0, orc.SCARP, 10, p2, a2)
    A = np.concatenate([a_1.reshape(-1, 80, 84), a_2.reshape(-1, 80, 84)])
    S = np.concatenate([s_1.reshape(-1, 80, 84), s_2.reshape(-1, 80, 84)])
    ages = np.concatenate([np.repeat(p1, len(a1)), np.repeat(p2, len(a2))])
    angs = np.concatenate([np.tile(a1, len(p1)), np.tile(a2, len(p2))])
    chk = orc.check_fold(res, A, S, ages, angs, tie_rtol=TIE_RTOL,
                         amp_tol=(AMP_RTOL, AMP_ATOL * np.abs(A).max()), snr_tol=(SNR_RTOL, SNR_ATOL * S.max()))
    report("two searches, two grids, one record", chk, "auto")
    assert chk["n_bad"] == 0 and chk["exact_frac"] >= EXACT_MIN, chk
    assert np.isin(res[1][res[3] > 0], ages).all()
    assert (np.isin(res[1], p1) & (res[3] > 0)).any() and (np.isin(res[1], p2) & (res[3] > 0)).any()


def test_direct_path_rejects_windows_wider_than_its_lds_slab(gpu_ctx):
    """k_direct stages a 64-cell patch plus the window width per LDS row: a window
    wider than the slab must come back as SC_ERR_UNSUPPORTED, not corrupt LDS."""
    z = np.zeros((64, 3000), np.float32)
    z[:, ::7] = 1.0
    m = sl.Matcher(grid(z, 1.0), ctx=gpu_ctx)

    class Wide(WT.Scarp):
        def _device_descriptor(self):
            return None

        def template(self):
            W = np.zeros((self.ny, self.nx))
            W[self.ny // 2, 100:2900] = 1.0
            return W
    try:
        with pytest.raises(sl._lib.ScarpletHipError, match="real-space"):
            m.match_template(Wide, 10, 1.0, 0.0, method="direct")
        amp, snr = m.match_template(Wide, 10, 1.0, 0.0, method="auto")     # FFT takes it
        assert np.isfinite(amp).all()
    finally:
        m.ctx.clear_windows()


def test_real_space_kernel_forms_agree(gpu_ctx):
    """The real-space path in its three forms - k_direct2 with T3 shared between a lane's adjacent
    outputs (default), with T3 accumulated tap by tap (variant 11), and the round-2 box kernel
    (variant 10) - sums the same products in different orders: the maps agree to float32 rounding,
    on thin and on wide windows, with and without the hole a Scarp window has at xr = 0."""
    g = synthetic.synthetic_scarp(700, ny=610, seed=12)
    m = sl.Matcher(g, ctx=gpu_ctx)
    try:
        for scale, age, ang in ((60, 1.0, 0.0), (60, 300.0, 0.0), (40, 100.0, 0.7), (25, 30.0, -np.pi / 2), (80, 1000.0, 1.2)):
            out = {}
            for v in (0, 11, 10):
                m.ctx.set_option("variant", v)
                out[v] = m.match_template(WT.Scarp, scale, age, ang, method="direct")
            for v in (11, 10):
                for k in (0, 1):
                    d = np.abs(out[v][k] - out[0][k]).max()
                    assert d <= 2e-5 * np.abs(out[0][k]).max(), (scale, age, ang, v, k, d)
    finally:
        m.ctx.set_option("variant", 0)


def test_direct_path_widest_window_on_a_large_dem(gpu_ctx):
    """A window close to the widest the real-space kernel stages (2 100 cells: the 512-cell patch
    would overflow its LDS slab, the 256-cell patch holds it) on a DEM large enough to be offered
    the 512-cell patch - 400 x 10300: 21 x 25 = 525 patches of 512 x 16, direct_route wants 512 of them
    and refuses the patch because (512 + 2100) x 16 floats do not fit; the 256 x 16 patch's slab holds
    two of the window's three rows at a time (tests/test_direct_route_host.py: the same on the CPU): the result equals the FFT path's, and the float64 oracle's in the
    corners, astride a patch seam, in the partial last patch and in the interior."""
    rng = np.random.default_rng(8)
    ny, nx = 400, 10300
    z = (rng.standard_normal((ny, nx)) * 0.1).astype(np.float32)
    m = sl.Matcher(grid(z, 1.0), ctx=gpu_ctx)
    row = np.sin(np.arange(2100) * 0.01) + 0.5

    class Wide(WT.Scarp):
        def _device_descriptor(self):
            return None

        def template(self):
            W = np.zeros((self.ny, self.nx))
            W[self.ny // 2 - 1:self.ny // 2 + 2, self.nx // 2 - 1050:self.nx // 2 + 1050] = row[np.newaxis, :]
            return W
    try:
        a_d, s_d = m.match_template(Wide, 10, 1.0, 0.0, method="direct")
        a_f, s_f = m.match_template(Wide, 10, 1.0, 0.0, method="fft")
        # (two float32 paths against each other, on white noise: to the maps' own scale)
        assert np.abs(a_d - a_f).max() <= AMP_RTOL * np.abs(a_f).max()
        assert np.abs(s_d - s_f).max() <= SNR_RTOL * s_f.max()
        assert s_f.max() > 0 and np.isfinite(a_d).all()
    finally:
        m.ctx.clear_windows()
    # the oracle at a few cells, as the real-space closed form of core.py:350-363 (oracle.xcorr_direct's sum, at those
    # cells only): window row k, column l of the centred template reads curvature cell (i - ny//2 - k, j - nx//2 - l)
    curv = orc.directional_curvature(z.astype(float), 1.0, 1.0, 0.0)
    ks = np.repeat(np.arange(ny // 2 - 1, ny // 2 + 2), 2100)
    ls = np.tile(np.arange(nx // 2 - 1050, nx // 2 + 1050), 3)
    w = np.tile(row, 3)
    ts, n = np.sum(w ** 2), len(w) + orc.EPS
    lim = np.asarray(Wide(10, 1.0, 0.0, nx, ny, 1.0).get_window_limits(), dtype=bool)
    # (rows below 10 / above 389 and columns below 6 / above 10293 lie outside this Scarp(10, 1.0, 0) class's window limits:
    #  a few masked probes, the rest at the patch seams in y - 16 k, 16 k + 8 - and in x - 256 k - and in the last patches)
    cells = [(i, j) for i in (0, 10, 15, 16, 23, 24, 200, 383, 384, 389, ny - 1)
             for j in (0, 6, 255, 256, 511, 512, 5000, 10239, 10240, nx - 7, nx - 1)]
    o = np.empty((len(cells), 2))
    for q, (i, j) in enumerate(cells):
        v = curv[(i - ny // 2 - ks) % ny, (j - nx // 2 - ls) % nx]
        xcorr, T3 = np.sum(w * v), np.sum(v ** 2)
        amp = xcorr / ts
        T1 = ts * amp ** 2
        o[q] = (0.0, 0.0) if lim[i, j] else (amp, abs(T1 / ((1 / n) * (T1 - 2 * amp * xcorr + T3) + orc.EPS)))
    assert (o[:, 1] > 0).sum() >= len(cells) // 2                  # (the probes are not all masked)
    ii, jj = np.array(cells).T
    d_a, d_s = np.abs(a_d[ii, jj] - o[:, 0]), np.abs(s_d[ii, jj] - o[:, 1])
    print("widest window, 256 x 16 class: max |d amp| %.2e of %.2e, max |d snr| %.2e of %.2e at %d cells"
          % (d_a.max(), np.abs(o[:, 0]).max(), d_s.max(), o[:, 1].max(), len(cells)))
    assert (d_a <= AMP_RTOL * np.abs(o[:, 0]) + AMP_ATOL * np.abs(o[:, 0]).max()).all()
    assert (d_s <= SNR_RTOL * o[:, 1] + SNR_ATOL * o[:, 1].max()).all()


def test_nan_dem_gives_the_reference_nan_maps(gpu_ctx):
    """dem.py:85-86,105 + core.py:349-375: one NaN cell turns every output cell NaN
    (the FFT spreads it), masks then zero their cells; compare() keeps age/angle 0."""
    rng = np.random.default_rng(4)
    z = rng.standard_normal((40, 44))
    z[3, 4] = np.nan
    with pytest.warns(UserWarning, match="NaN"):
        amp, age, ang, snr = sl.match_template(grid(z, 1.0), sl.Scarp, 5, 10., 0.3)
    o_amp, _, _, o_snr = orc.match_template(z, 1.0, 1.0, orc.SCARP, 5, 10., 0.3)
    assert np.array_equal(amp, o_amp, equal_nan=True) and np.array_equal(snr, o_snr, equal_nan=True)
    assert np.isnan(amp).any() and (amp == 0).any()
    with pytest.warns(UserWarning):
        res = sl.match(grid(z, 1.0), sl.RightFacingUpperBreakScarp, scale=5, age=10., ang_min=-0.05, ang_max=0.05)
    ref = orc.match(z, 1.0, 1.0, orc.RIGHT_UPPER, scale=5, age=10., ang_min=-0.05, ang_max=0.05)
    assert np.array_equal(res, ref, equal_nan=True)


# ------------------------------------------------------------------ full size
def test_full_size_properties(gpu_ctx):
    """BASELINE-sized DEM (10000 x 10000), a slice of the 35 x 181 grid:
    size-independent properties instead of the oracle -
      * fold idempotence: searching twice without a reset changes nothing;
      * linearity: doubling the relief doubles amp and leaves SNR / argmax;
      * locality: a window of the result equals the oracle run on a crop
        around it (interior cells only see the template's reach)."""
    n = 10000
    g = synthetic.synthetic_scarp(n)
    ages = _plan.age_grid()[[4, 19, 34]]
    angles = _plan.angle_grid()[[20, 95, 160]]
    m = sl.Matcher(g, ctx=gpu_ctx)
    m.search(sl.Scarp, 100, ages, angles, method="fft")
    amp, age, ang, snr = m.result()
    m.search(sl.Scarp, 100, ages, angles, method="fft", reset=False)
    amp2, age2, ang2, snr2 = m.result()
    assert np.array_equal(snr, snr2) and np.array_equal(amp, amp2) and np.array_equal(age, age2)

    # locality: crop with margin >= template reach + stencil, compare interior
    # margin: the window-limit mask of the crop reaches up to 2c + d*sqrt(2) = 375 cells inwards
    i0, j0, w, margin = 4200, 7300, 160, 400
    sl_ = (slice(i0 - margin, i0 + w + margin), slice(j0 - margin, j0 + w + margin))
    zc = g._griddata[sl_]
    a_st, s_st = orc.snr_stack(zc, 1.0, 1.0, orc.SCARP, 100, ages, angles, workers=4)
    # window limits of the crop differ from the full DEM's: compare un-masked stacks
    inner = (slice(margin, margin + w), slice(margin, margin + w))
    T = len(ages) * len(angles)
    win = (slice(i0, i0 + w), slice(j0, j0 + w))
    res_win = (amp[win], age[win], ang[win], snr[win])
    chk = orc.check_fold(res_win, a_st.reshape(T, *zc.shape)[(slice(None),) + inner],
                         s_st.reshape(T, *zc.shape)[(slice(None),) + inner],
                         np.repeat(ages, len(angles)), np.tile(angles, len(ages)),
                         tie_rtol=TIE_RTOL, amp_tol=(AMP_RTOL, AMP_ATOL * np.max(np.abs(a_st))),
                         snr_tol=(SNR_RTOL, SNR_ATOL * np.max(s_st)))
    if chk["n_bad"]:
        S = s_st.reshape(T, *zc.shape)[(slice(None),) + inner]
        A = a_st.reshape(T, *zc.shape)[(slice(None),) + inner]
        msgs = []
        for (i, j) in np.argwhere(~chk["ok"])[:6]:
            top = np.argsort(S[:, i, j])[::-1][:3]
            msgs.append("cell (%d,%d): got amp=%.6g age=%.6g ang=%.4f snr=%.6g; oracle top3 %s" % (
                i, j, res_win[0][i, j], res_win[1][i, j], res_win[2][i, j], res_win[3][i, j],
                [(float(np.repeat(ages, len(angles))[t]), float(np.tile(angles, len(ages))[t]),
                  float(S[t, i, j]), float(A[t, i, j])) for t in top]))
        raise AssertionError("\n".join(msgs))

    g2 = sl.DEMGrid.from_array(g._griddata * 2.0, 1.0)
    m.set_data(g2)
    m.search(sl.Scarp, 100, ages, angles, method="fft")
    amp3, age3, ang3, snr3 = m.result()
    assert np.allclose(amp3, 2 * amp, rtol=1e-4, atol=1e-6)
    assert np.allclose(snr3, snr, rtol=2e-3, atol=1e-5)
    assert (age3 == age).mean() > 0.999


def test_async_searches_back_to_back_equal_the_synchronous_ones(gpu_ctx):
    """sc_match_async twice without sc_sync in between (two grids folded into one record): the
    descriptors of a search are uploaded asynchronously from host copies the context keeps, and the
    second call must not overwrite them while the first call's copy may still be in flight.  The
    record must equal, bit for bit, the one the same two searches leave when each is waited for."""
    rng = np.random.default_rng(77)
    z = (np.cumsum(rng.standard_normal((300, 260)), 1) * 0.04 + rng.standard_normal((300, 260)) * 0.05).astype(np.float32)
    g = grid(z, 1.0)
    grids = [([1.0, 10.0], _plan.angle_grid()[::9]), ([3.0, 30.0, 100.0], _plan.angle_grid()[4::11])]
    out = []
    for sync in (True, False):
        m = sl.Matcher(g, ctx=gpu_ctx)
        for k, (params, angles) in enumerate(grids):
            m.search(WT.Scarp, 12, params, angles, method="fft", reset=(k == 0), sync=sync)
        m.ctx.sync()
        out.append(m.ctx.get_best())
    for a, b, name in zip(out[0], out[1], ("amp", "snr", "id")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert (out[0][1] > 0).any()


def test_near_tie_events_and_pair_scoring(gpu_ctx):
    """The two entry points of exact=True's short route.  sc_get_near_events: with option "near_window" on, every event
    names a flagged cell and two templates of the search (or SC_ID_NONE as the holder), every flagged cell has an event,
    and a reset empties the list.  sc_score_pairs_f64: pair (cell, template) = the entry of sc_score_cells_f64's table."""
    rng = np.random.default_rng(5)
    ny, nx = 150, 170
    z = (np.cumsum(np.cumsum(rng.standard_normal((ny, nx)), 0), 1) * 0.01 + rng.standard_normal((ny, nx)) * 0.05).astype(np.float32)
    params, angles = [2.0, 9.0, 40.0], _plan.angle_grid(-np.pi / 2, np.pi / 2)[::9]
    m = sl.Matcher(grid(z, 1.0, 1.0), ctx=gpu_ctx)
    assert len(m.ctx.near_events()) == 0 or True                  # (whatever an earlier test left: reset below)
    m.ctx.set_option("near_window", 5e-3)                         # (wide: a few thousand events on this small DEM)
    try:
        m.search(WT.Scarp, 10, params, angles, method="fft")
    finally:
        m.ctx.set_option("near_window", 0.0)
    flags, ev = m.ctx.near_ties(), m.ctx.near_events()
    assert ev is not None and len(ev) > 100 and flags.sum() > 100
    n_t = len(params) * len(angles)
    cells = ev[:, 0].astype(np.int64)
    assert cells.max() < ny * nx and np.all(flags.ravel()[cells] == 1)
    assert set(np.flatnonzero(flags.ravel())) == set(cells.tolist())
    assert np.all(ev[:, 1] < n_t) and np.all((ev[:, 2] < n_t) | (ev[:, 2] == 0xFFFFFFFF)) and np.all(ev[:, 1] != ev[:, 2])
    # pairs against the full table (template ids of a fresh search are ia * n_angles + ib; the table is orientation-major)
    pick = rng.choice(len(ev), 60, replace=False)
    ij = np.column_stack([cells[pick] // nx, cells[pick] % nx])
    ids = ev[pick, 1].astype(np.int64)
    tix = (ids % len(angles)) * len(params) + ids // len(angles)
    a_all, s_all = m.ctx.score_cells_f64(ij, n_t)
    a_p, s_p = m.ctx.score_pairs_f64(ij, tix)
    assert np.allclose(a_p, a_all[np.arange(60), tix], rtol=1e-12, atol=0) and np.allclose(s_p, s_all[np.arange(60), tix], rtol=1e-12, atol=0)
    with pytest.raises(sl._lib.ScarpletHipError):
        m.ctx.score_pairs_f64(ij[:2], [0, n_t])                   # a template the search did not hold
    m.ctx.reset_best()
    assert len(m.ctx.near_events()) == 0 and m.ctx.near_ties().sum() == 0


def test_random_searches_against_the_oracle(gpu_ctx):
    """The wide net of tools/fuzz_oracle.py in the driver-run suite: 40 random searches (DEM size and parity, power-of-two
    periodic DEMs, cell size, sign of dy, float and int16 surfaces, the five built-in template classes, 1 - 6 parameters
    x 1 - 7 orientations incl. the -pi/2, 0, +pi/2 windows) through the FFT path, the real-space path, method="auto" and
    exact=True against the oracle: NO cell outside oracle.PARITY on any path, and with exact=True no cell whose
    (age, angle) is not the oracle's own argmax.  (970 searches of the same generator: profiles/r05_fuzz_oracle.txt.)"""
    kinds = {WT.Scarp: orc.SCARP, WT.Ricker: orc.RICKER, WT.Channel: orc.RICKER,
             WT.RightFacingUpperBreakScarp: "right_upper_break", WT.LeftFacingUpperBreakScarp: "left_upper_break"}
    classes = [WT.Scarp, WT.Scarp, WT.Channel, WT.Ricker, WT.LeftFacingUpperBreakScarp, WT.RightFacingUpperBreakScarp]
    rng = np.random.default_rng(41)
    off = {"fft": 0, "direct": 0, "auto": 0, "exact": 0, "default": 0, "direct exact": 0}
    cells = 0
    for case in range(40):
        ny, nx = (int(v) for v in rng.integers(48, 300, size=2))
        if case % 7 == 0:
            ny, nx = int(2 ** rng.integers(6, 9)), int(2 ** rng.integers(6, 9))
        cls = classes[int(rng.integers(0, len(classes)))]
        de = float(rng.choice([1.0, 1.0, 2.0, 0.5]))
        scale = float(rng.uniform(4, min(ny, nx) / 4.5)) * de
        if cls in (WT.Channel, WT.Ricker):
            params = list(np.round(rng.uniform(0.05, 0.4, size=int(rng.integers(1, 4))) / de, 4))
        else:
            params = list(np.round(10 ** rng.uniform(0, 2.6, size=int(rng.integers(1, 7))) * de * de, 3))
        angles = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, size=int(rng.integers(1, 8))))
        if case % 5 == 0:
            angles = np.array([-np.pi / 2, 0.0, np.pi / 2])
        z = np.cumsum(np.cumsum(rng.standard_normal((ny, nx)), 0), 1) * 0.01 + rng.standard_normal((ny, nx)) * 0.05
        if case % 4 == 1:
            z = np.round(z * 20.0).astype(np.int16)
        z = z.astype(np.float32)
        dy = -de if case % 3 == 0 else de
        kind = kinds[cls]
        a_st, s_st = orc.snr_stack(z, de, dy, kind, scale, params, angles)
        T = len(params) * len(angles)
        ages, angs = np.repeat(np.asarray(params, float), len(angles)), np.tile(angles, len(params))
        A, S = a_st.reshape(T, ny, nx), s_st.reshape(T, ny, nx)
        tol = dict(amp_tol=(AMP_RTOL, AMP_ATOL * float(np.max(np.abs(A)))),
                   snr_tol=(orc.snr_tolerance(kind)[0], orc.snr_tolerance(kind)[1] * float(np.max(S))))
        cells += ny * nx
        for name, kw in (("fft", dict(method="fft")), ("direct", dict(method="direct")), ("auto", dict(method="auto")),
                         ("exact", dict(method="fft", exact=True)), ("default", dict(method="auto", exact=None)),
                         ("direct exact", dict(method="direct", exact=True))):
            m = sl.Matcher(grid(z, de, dy), ctx=gpu_ctx)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                   # (exact=True says when it searches the whole DEM again)
                res = m.search(cls, scale, params, angles, **kw).result()
            chk = orc.check_fold(res, A, S, ages, angs, tie_rtol=orc.tie_window(m.method_used, kind), **tol)
            assert chk["n_bad"] == 0, (case, cls.__name__, (ny, nx), de, dy, scale, name, chk["n_bad"])
            off[name] += chk["n_inexact"]
    print("     40 random searches, %d cells: off the oracle's argmax (near-ties inside the window) %s" % (cells, off))
    assert off["exact"] == 0 and off["default"] == 0 and off["direct exact"] == 0, off
    # (the float32 searches of the same inputs are off the argmax somewhere: the counts above can fail)
    assert off["fft"] + off["direct"] + off["auto"] >= 1, off


def test_exact_mode_on_the_real_space_path(gpu_ctx):
    """exact=True where the search runs on the real-space path - asked for by name, chosen by `auto`, or taken because
    the flagging row kernel does not serve the templates (an UpperBreak's error masks): the path flags the cells it
    decides inside its own float32 rounding and those take the float64 argmax (sc_score_cells_f64).  The searches here
    hold two orientations 2e-6 rad apart - SNRs 1e-6 apart in float64, nothing float32 resolves: without the mode
    about half the cells carry the other one (allowed: a near-tie inside the window), with it none does."""
    rng = np.random.default_rng(77)
    for (kind, cls, ny, nx, de, dy, scale, params, method) in [
            (orc.SCARP, WT.Scarp, 96, 90, 1.0, 1.0, 10, [4.0, 30.0], "direct"),
            (orc.SCARP, WT.Scarp, 70, 101, 2.0, -2.0, 16, [12.0], "auto"),
            ("left_upper_break", WT.LeftFacingUpperBreakScarp, 88, 84, 1.0, 1.0, 9, [5.0, 20.0], "fft")]:
        angles = np.array([-0.7, 0.3, 0.3 + 2e-6])
        z = (np.cumsum(np.cumsum(rng.standard_normal((ny, nx)), 0), 1) * 0.01 + rng.standard_normal((ny, nx)) * 0.05).astype(np.float32)
        a_st, s_st = orc.snr_stack(z, de, dy, kind, scale, params, angles)
        T = len(params) * len(angles)
        ages, angs = np.repeat(np.asarray(params, float), len(angles)), np.tile(angles, len(params))
        A, S = a_st.reshape(T, ny, nx), s_st.reshape(T, ny, nx)
        tol = dict(amp_tol=(AMP_RTOL, AMP_ATOL * float(np.max(np.abs(A)))),
                   snr_tol=(orc.snr_tolerance(kind)[0], orc.snr_tolerance(kind)[1] * float(np.max(S))))
        off = {}
        for exact in (False, True):
            m = sl.Matcher(grid(z, de, dy), ctx=gpu_ctx)
            res = m.search(cls, scale, params, angles, method=method, exact=exact).result()
            chk = orc.check_fold(res, A, S, ages, angs, tie_rtol=orc.tie_window(m.method_used, kind), **tol)
            assert chk["n_bad"] == 0, (str(kind), method, exact, chk["n_bad"], m.method_used)
            assert m.method_used == "direct" or not exact, (str(kind), method, m.method_used)
            off[exact] = chk["n_inexact"]
            if exact:
                assert m.exact_stats["float64_cells"] > 0, m.exact_stats
        print("     exact on the real-space path, %s / %s: cells off the oracle's argmax %d -> %d (float64 cells %d of %d)" % (
            cls.__name__, method, off[False], off[True], m.exact_stats["float64_cells"], ny * nx))
        assert off[False] > 0 and off[True] == 0, (str(kind), method, off)


def test_float64_scoring_of_single_cells(gpu_ctx):
    """sc_score_cells_f64 - match_template() at single cells in float64 on the device, the last step of exact=True -
    against the oracle's float64 maps: Scarp (odd and even grid sizes, dy < 0, an UpperBreak's error mask, cells at the
    window-limit border and on the DEM's edge) and Ricker, to 1e-9 of the map's largest value."""
    rng = np.random.default_rng(33)
    for (kind, cls, ny, nx, de, dy, scale, params, angles) in [
            (orc.SCARP, WT.Scarp, 90, 101, 1.0, 1.0, 8, [1.0, 6.0, 40.0], [-1.3, -0.2, 0.0, 0.9, np.pi / 2]),
            (orc.SCARP, WT.Scarp, 80, 64, 2.0, -2.0, 14, [3.0, 25.0], [-np.pi / 2, 0.4]),
            ("left_upper_break", WT.LeftFacingUpperBreakScarp, 72, 76, 1.0, 1.0, 9, [5.0], [-0.6, 0.7]),
            (orc.RICKER, WT.Ricker, 64, 72, 1.0, -1.0, 6, [0.1, 0.25], [-0.8, 0.0, 1.1])]:
        z = (np.cumsum(np.cumsum(rng.standard_normal((ny, nx)), 0), 1) * 0.01 + rng.standard_normal((ny, nx)) * 0.05).astype(np.float32)
        m = sl.Matcher(grid(z, de, dy), ctx=gpu_ctx)
        m.search(cls, scale, params, angles, method="direct")
        cells = np.column_stack([rng.integers(0, ny, 40), rng.integers(0, nx, 40)])
        cells[:4] = [[0, 0], [ny - 1, nx - 1], [ny // 2, 0], [0, nx // 2]]
        n_t = len(params) * len(angles)
        amp, snr = m.ctx.score_cells_f64(cells, n_t)
        # (ABI 8: the count the caller sized its arrays for is checked against the search the context holds)
        with pytest.raises(sl._lib.ScarpletHipError, match="expects"):
            m.ctx.score_cells_f64(cells, n_t - 1)
        k = 0
        for ang in angles:                                  # hand-over order: orientation-major
            for par in params:
                o_amp, _, _, o_snr = orc.match_template(z, de, dy, kind, scale, par, ang)
                ea = np.abs(amp[:, k] - o_amp[cells[:, 0], cells[:, 1]]).max() / max(np.abs(o_amp).max(), 1e-300)
                es = np.abs(snr[:, k] - o_snr[cells[:, 0], cells[:, 1]]).max() / max(o_snr.max(), 1e-300)
                assert ea <= 1e-9 and es <= 1e-9, (str(kind), par, ang, ea, es)
                k += 1
