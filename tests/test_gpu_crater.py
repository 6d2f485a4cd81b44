"""sl.match_craters on the MI355X (docs/craters.md): the windows sc_crater_windows synthesises against the reference's
Crater.template() (tests/golden/ref_crater.npz), and the (radius, age) search against the float64 oracle -
orc.match_arrays over the Laplacian d2z_dx2 + d2z_dy2, the golden-checked numpy class and the limit rectangle, folded
by orc.compare in the device's order (radius-major)."""
import warnings

import numpy as np
import pytest

import scarplet_oracle as orc
import scarplet_amd as sl
from scarplet_amd import WindowedTemplate as WT
from test_crater_host import golden_cases

pytestmark = pytest.mark.gpu

RADII = [6.0, 10.0, 20.0]
AGES = [1.0, 3.0, 10.0, 30.0]


def grid(z, de):
    return sl.DEMGrid.from_array(np.asarray(z), float(de))


# ---- the windows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_device_windows_are_the_reference(gpu_ctx, k):
    (r, kt, nx, ny, de), gold = golden_cases()[k]
    sl.Matcher(grid(np.zeros((ny, nx)), de), ctx=gpu_ctx)
    tables = WT.crater_tables([r], [kt], nx, ny, de)
    try:
        slots, count, sumsq, wins = gpu_ctx.crater_windows(tables, return_windows=True)
        raw = wins[0].tobytes(), count.tobytes(), sumsq.tobytes()
        again = gpu_ctx.crater_windows(tables, return_windows=True)
    finally:
        gpu_ctx.clear_windows()
    pmin, pmax, qmin, qmax = (int(v) for v in tables["boxes"][0])
    assert wins[0].shape == (pmax - pmin + 1, qmax - qmin + 1) and len(slots) == 1 and again[0][0] != slots[0]
    W = np.zeros((ny, nx))
    W[ny // 2 + pmin:ny // 2 + pmax + 1, nx // 2 + qmin:nx // 2 + qmax + 1] = wins[0]
    assert np.array_equal(W != 0, gold != 0), int(((W != 0) != (gold != 0)).sum())
    err = np.abs(W - gold).max() / np.abs(gold).max()
    rel = abs(sumsq[0] - np.sum(gold ** 2)) / np.sum(gold ** 2)
    print("case %d: %d cells, max |dW| / max |W| = %.2e, sum(W^2) off by %.2e" % (k, int(count[0]), err, rel))
    assert err <= 1e-13
    assert count[0] == np.count_nonzero(gold)
    assert rel <= 1e-12
    assert (again[3][0].tobytes(), again[1].tobytes(), again[2].tobytes()) == raw


def test_windows_of_a_grid_of_radii_and_ages(gpu_ctx):
    """Several radii and ages in one call: template k = i_radius * n_ages + i_age, each the numpy class's window."""
    ny, nx, de = 90, 101, 1.0
    sl.Matcher(grid(np.zeros((ny, nx)), de), ctx=gpu_ctx)
    tables = WT.crater_tables(RADII, AGES, nx, ny, de)
    try:
        slots, count, sumsq, wins = gpu_ctx.crater_windows(tables, return_windows=True)
    finally:
        gpu_ctx.clear_windows()
    assert list(slots) == list(range(12))
    for ib, r in enumerate(RADII):
        pmin, pmax, qmin, qmax = (int(v) for v in tables["boxes"][ib])
        for ia, kt in enumerate(AGES):
            ref = WT.Crater(r, kt, nx, ny, de).template()
            box = ref[ny // 2 + pmin:ny // 2 + pmax + 1, nx // 2 + qmin:nx // 2 + qmax + 1]
            w = wins[ib * len(AGES) + ia]
            assert np.count_nonzero(ref) == np.count_nonzero(box) == count[ib * len(AGES) + ia]
            assert np.array_equal(w != 0, box != 0) and np.abs(w - box).max() <= 1e-13 * np.abs(box).max()


def test_a_box_that_leaves_the_grid_is_a_value_error(gpu_ctx):
    sl.Matcher(grid(np.zeros((40, 44)), 1.0), ctx=gpu_ctx)
    tables = WT.crater_tables([20.0], [1.0], 100, 100, 1.0)            # made for a larger grid
    with pytest.raises(ValueError, match="leaves the 40 x 44 grid"):
        gpu_ctx.crater_windows(tables)
    gpu_ctx.clear_windows()


# ---- the search ----------------------------------------------------------------------------------------------------------
def bowl_dem(shape, de, centre, r_cells, seed):
    """Seeded Gaussian noise plus one bowl with a raised rim of radius ``r_cells`` about ``centre``."""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[:shape[0], :shape[1]].astype(float)
    rho = np.hypot(i - centre[0], j - centre[1]) * de
    R = r_cells * de
    z = 0.6 * np.exp(-0.5 * ((rho - R) / (0.25 * R)) ** 2) + np.where(rho < R, 0.5 * ((rho / R) ** 2 - 1.0), 0.0)
    return (z + 0.02 * rng.standard_normal(shape)).astype(np.float32)


DEMS = {"96x80": dict(shape=(96, 80), de=1.0, centre=(50, 41), r_cells=10, seed=11),
        "129x100": dict(shape=(129, 100), de=2.0, centre=(66, 52), r_cells=5, seed=12)}


class _Case(object):
    def __init__(self, name):
        d = DEMS[name]
        self.de, self.centre = d["de"], d["centre"]
        self.z = bowl_dem(d["shape"], d["de"], d["centre"], d["r_cells"], d["seed"])
        ny, nx = self.z.shape
        A, _, C = orc.curvature_components(self.z, self.de, self.de)
        curv = A + C
        amps, snrs, results, lims = [], [], [], []
        for r in RADII:                                   # the device's fold order: radius-major
            for kt in AGES:
                t = WT.Crater(r, kt, nx, ny, self.de)
                lim = t.get_window_limits()
                a, s = orc.match_arrays(curv, t.template(), lim)
                amps.append(a)
                snrs.append(s)
                lims.append(lim)
                results.append((a, kt, r, s))
        self.amp, self.snr = np.stack(amps), np.stack(snrs)
        self.t_age, self.t_rad = np.tile(AGES, len(RADII)), np.repeat(RADII, len(AGES))
        self.fold = np.stack(orc.compare(results, ny, nx))
        self.masked = np.all(lims, axis=0)


_CASES = {}


@pytest.fixture(params=sorted(DEMS))
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = _Case(request.param)
    return _CASES[request.param]


def _search(gpu_ctx, c, method, exact):
    m = sl.Matcher(grid(c.z, c.de), ctx=gpu_ctx)
    try:
        res = np.array(m.search_craters(RADII, AGES, method=method, exact=exact).result_array())
    finally:
        gpu_ctx.clear_windows()
    return m, res


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_float32_search_against_the_oracle(gpu_ctx, case, method):
    c = case
    m, res = _search(gpu_ctx, c, method, False)
    assert m.method_used == method
    P = orc.PARITY
    rtol, afac = orc.snr_tolerance()
    tw = orc.tie_window(method)
    chk = orc.check_fold(res, c.amp, c.snr, c.t_age, c.t_rad, tie_rtol=tw,
                         amp_tol=(P["amp"][0], P["amp"][1] * np.abs(c.amp).max()), snr_tol=(rtol, afac * c.snr.max()))
    top = np.sort(c.snr, axis=0)
    led = (top[-1] > 0) & (top[-1] - top[-2] > tw * top[-1])        # the oracle's winner leads by more than the tie window
    print("%s %s: %d cells, %d led, %d bad; max rel SNR error %.2e, amp %.2e (tolerances %.0e, %.0e)"
          % (c.z.shape, method, chk["n"], int(led.sum()), chk["n_bad"], chk["snr_err"], chk["amp_err"], rtol, P["amp"][0]))
    assert led.sum() > 0.5 * (~c.masked).sum()
    assert chk["ok"][led].all(), np.argwhere(led & ~chk["ok"])[:5]
    k = np.argmax(c.snr, axis=0)
    assert (res[1][led] == c.t_age[k][led]).all() and (res[2][led] == c.t_rad[k][led]).all()
    assert chk["n_bad"] == 0, chk["n_bad"]
    # masked cells are zero in all four planes; plane 2 holds radii (or 0)
    assert c.masked.sum() > 0 and (res[:, c.masked] == 0).all()
    assert set(np.unique(res[2])) <= set(RADII) | {0.0}
    assert set(np.unique(res[1])) <= set(AGES) | {0.0}
    # the same bytes on every run
    _, again = _search(gpu_ctx, c, method, False)
    assert again.tobytes() == res.tobytes()


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_exact_search_is_the_float64_argmax(gpu_ctx, case, method):
    c = case
    m, res = _search(gpu_ctx, c, method, True)
    st = dict(m.exact_stats)
    kept = c.fold[3] > 0
    off = kept & ((res[1] != c.fold[1]) | (res[2] != c.fold[2]))
    print("%s %s (%s path): %d kept cells, %d off the float64 argmax; exact_stats %s"
          % (c.z.shape, method, m.method_used, int(kept.sum()), int(off.sum()), st))
    assert st.get("route") == "device" and "skipped" not in st, st
    assert kept.sum() == (~c.masked).sum()
    assert off.sum() == 0, np.argwhere(off)[:5]
    assert (res[:, c.masked] == 0).all() and (res[3][kept] > 0).all()
    # the planted bowl: at its centre the device's (age, radius) is the oracle's (what they are: docs/craters.md)
    i, j = c.centre
    print("     planted bowl at %s: (age, radius) = (%g, %g), SNR %.1f" % (c.centre, res[1][i, j], res[2][i, j], res[3][i, j]))
    assert (res[1][i, j], res[2][i, j]) == (c.fold[1][i, j], c.fold[2][i, j]) and kept[i, j]
    _, again = _search(gpu_ctx, c, method, True)
    assert again.tobytes() == res.tobytes()


def test_match_craters_is_the_search(gpu_ctx, case):
    c = case
    res = sl.match_craters(grid(c.z, c.de), RADII, AGES, method="direct", exact=False)
    _, want = _search(gpu_ctx, c, "direct", False)
    assert res.shape == (4,) + c.z.shape and res.dtype == np.float64 and res.tobytes() == want.tobytes()


def test_a_dem_with_nan_cells_is_answered_as_match_answers_it(gpu_ctx):
    c = _Case("96x80")
    z = c.z.copy()
    z[10, 10] = np.nan
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = sl.match_craters(grid(z, c.de), RADII, AGES)
    assert any("NaN" in str(w.message) for w in caught)
    kept = ~c.masked
    assert np.isnan(res[0][kept]).all() and np.isnan(res[3][kept]).all()
    assert (res[0][c.masked] == 0).all() and (res[3][c.masked] == 0).all() and (res[1] == 0).all() and (res[2] == 0).all()
