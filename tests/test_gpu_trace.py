"""Traces of a result on the MI355X (sc_trace_planes / sc_trace_result, docs/traces.md) against the numpy reference
(tests/trace_reference.py): random planes with ties, NaN cells and boundary angles, real search results, the
direction convention checked on synthetic scarps, determinism, both routes, and no side effects on the search."""
import numpy as np
import pytest

import scarplet_amd as sl
import trace_reference as tr
from scarplet_amd import _lib, _plan, synthetic
from test_gpu_configs import dem_fixture
from test_gpu_parity import grid

pytestmark = pytest.mark.gpu


def random_planes(ny, nx, seed):
    rng = np.random.default_rng(seed)
    snr = rng.lognormal(0.0, 1.0, (ny, nx))
    # exact ties: runs of equal values along rows and columns, and a few repeated values everywhere
    k = max(1, ny * nx // 20)
    r, c = rng.integers(0, ny, k), rng.integers(0, nx, k)
    snr[r, c] = snr[r, np.minimum(c + 1, nx - 1)]
    r, c = rng.integers(0, ny, k), rng.integers(0, nx, k)
    snr[r, c] = snr[np.minimum(r + 1, ny - 1), c]
    snr[rng.random((ny, nx)) < 0.05] = 2.0
    ang = rng.uniform(-5 * np.pi, 5 * np.pi, (ny, nx))
    sel = rng.random((ny, nx)) < 0.05
    ang[sel] = rng.integers(-12, 13, sel.sum()) * (np.pi / 8)          # exact sector boundaries
    snr[rng.random((ny, nx)) < 0.005] = np.nan
    ang[rng.random((ny, nx)) < 0.005] = np.nan
    snr[rng.random((ny, nx)) < 0.01] = 0.0                            # (zeroed margins)
    amp = rng.standard_normal((ny, nx))
    age = 10 ** rng.uniform(0, 3.5, (ny, nx))
    return np.stack([amp, age, ang, snr])


def check(got, planes, snr_low, snr_high=None, min_cells=1):
    t, labels, ref = tr.trace(planes, snr_low, snr_high, min_cells)
    assert got.thin.dtype == bool and np.array_equal(got.thin, t)
    assert got.labels.dtype == np.int32 and np.array_equal(got.labels, labels)
    seg = got.segments
    K = len(ref["first"])
    assert len(seg) == K
    assert np.array_equal(seg["label"], np.arange(1, K + 1))
    for f in tr.INT_FIELDS:
        assert np.array_equal(seg[f], ref[f]), f
    for f in tr.PEAK_FIELDS:
        assert np.array_equal(seg[f], ref[f]), f                       # copied exactly
    for f in tr.SUM_FIELDS:
        if K:
            assert np.all(np.abs(seg[f] - ref[f]) <= 1e-12 * ref[f + "_abs"]), f
    if K:
        assert np.array_equal(seg["mean_snr"], seg["sum_snr"] / seg["n_cells"])
        assert np.array_equal(seg["strike"], 0.5 * np.arctan2(seg["sum_sin2a"], seg["sum_cos2a"]))
    return K


SETTINGS = [(1.0, None, 1), (2.0, 4.0, 3), (0.5, 8.0, 1), (1e9, None, 1)]


@pytest.mark.parametrize("shape", [(1, 1), (1, 257), (263, 1), (257, 263), (1000, 1000), (4096, 4096)])
def test_random_planes_against_reference(shape):
    p = random_planes(*shape, seed=shape[0] * 7919 + shape[1])
    ks = []
    for lo, hi, mc in SETTINGS:
        ks.append(check(sl.extract_traces(p, lo, hi, mc), p, lo, hi, mc))
    assert ks[-1] == 0                                                  # one setting yields no segment
    if shape[0] * shape[1] > 1000:
        assert min(ks[:-1]) > 0


def test_tuple_input_and_one_cell_segments():
    p = random_planes(300, 200, 5)
    got = sl.extract_traces(tuple(p), 1.0)
    check(got, p, 1.0)
    assert got.segments["n_cells"].min() == 1


def test_real_results_against_reference():
    z, dx, dy = dem_fixture("dem_carrizo.npz")
    res = np.stack(sl.match(grid(z, dx, dy), sl.Scarp, scale=100.))    # the reference's flagship call
    s = res[3][res[3] > 0]
    for lo, hi, mc in [(np.percentile(s, 50), np.percentile(s, 90), 5), (np.percentile(s, 90), None, 1)]:
        assert check(sl.extract_traces(res, lo, hi, mc), res, lo, hi, mc) > 0
    z, dx, dy = dem_fixture("dem_grandcanyon.npz")
    res = sl.match(grid(z, dx, dy), sl.Channel, scale=10., age=0.1, ang_min=-np.pi / 2, ang_max=np.pi / 2)
    s = res[3][res[3] > 0]
    lo, hi = np.percentile(s, 70), np.percentile(s, 95)
    assert check(sl.extract_traces(res, lo, hi, 10), res, lo, hi, 10) > 0


@pytest.mark.parametrize("theta, sector", [(0.2, 0), (np.pi / 4, 1), (np.pi / 2 - 0.2, 2), (3 * np.pi / 4, 3)])
def test_direction_convention_on_synthetic_scarps(theta, sector):
    """The largest segment of a synthetic scarp lies on its line yrot = 0: thinning runs across the profile of the
    winning template.  A step table that runs along the strike instead leaves a segment of scattered plateau cells."""
    n = 1024
    res = np.stack(sl.match(synthetic.synthetic_scarp(n, theta=theta), sl.Scarp, scale=100.))
    smax = np.nanmax(res[3])
    out = sl.extract_traces(res, 0.2 * smax, 0.5 * smax, 50)
    assert len(out.segments)
    k = int(np.argmax(out.segments["n_cells"]))
    s = out.segments[k]
    rr, cc = np.nonzero(out.labels == s["label"])
    assert np.bincount(tr.sectors(res[2][rr, cc]), minlength=4).argmax() == sector
    x = np.linspace(-n / 2, n / 2, num=n)
    th = np.pi / 2 - theta
    yrot = -x[cc] * np.sin(th) + x[rr] * np.cos(th)
    far = np.mean(np.abs(yrot) > 2)
    span = (s["row_max"] - s["row_min"], s["col_max"] - s["col_min"])
    cheb = max(span) + 1
    # every step along the line is covered: one cell per row (per column) of the bounding box's longer side
    steps = len(np.unique(rr if span[0] >= span[1] else cc))
    print("theta %.3f: %d cells, Chebyshev length %d, %d steps, %.4f off the line" % (theta, s["n_cells"], cheb, steps, far))
    assert far <= 0.02
    assert abs(steps - cheb) <= 0.1 * cheb
    if sector in (0, 2):
        assert abs(s["n_cells"] - cheb) <= 0.1 * cheb
    else:
        # a diagonal step visits two interleaved lattices of cells: each can hold its own maximum next to the line
        assert s["n_cells"] <= 2.2 * cheb


def _search(m, exact):
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid(), exact=exact)
    return m


@pytest.mark.parametrize("exact", [True, False])
def test_routes_determinism_and_no_side_effects(exact):
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = _search(sl.Matcher(g), exact)
    before = np.array(m.result_array())
    lo, hi = np.percentile(before[3][before[3] > 0], [60, 90])
    a = m.extract_traces(lo, hi, 4)
    b = m.extract_traces(lo, hi, 4)
    c = sl.extract_traces(before, lo, hi, 4)
    for x in (b, c):
        assert np.array_equal(a.thin, x.thin) and np.array_equal(a.labels, x.labels)
        assert a.segments.tobytes() == x.segments.tobytes()
    assert len(a.segments) > 0
    check(a, before, lo, hi, 4)
    assert np.array_equal(np.array(m.result_array()), before, equal_nan=True)
    # a second search that starts from the kept spectra gives the same bits with the trace in between
    again = np.array(_search(m, exact).result_array())
    m2 = _search(sl.Matcher(g, ctx=_lib.Context(0)), exact)
    assert np.array_equal(again, np.array(m2.result_array()), equal_nan=True)
    assert np.array_equal(again, before, equal_nan=True)


def test_nan_dem_takes_the_host_route():
    z = np.asarray(synthetic.synthetic_scarp(128)._griddata, dtype=np.float64).copy()
    z[5, 7] = np.nan
    with pytest.warns(UserWarning):
        m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))
    m.search(sl.Scarp, 10., [10.], _plan.angle_grid(-0.2, 0.2))
    out = m.extract_traces(1.0)
    assert not out.thin.any() and len(out.segments) == 0


@pytest.mark.slow
def test_full_size_benchmark_result():
    m = sl.Matcher(synthetic.synthetic_scarp(10000))
    res = np.array(m.search(sl.Scarp, 100., _plan.age_grid(), _plan.angle_grid()).result_array())
    smax = np.nanmax(res[3])
    lo, hi = 0.2 * smax, 0.5 * smax
    a = m.extract_traces(lo, hi, 20)
    K = check(a, res, lo, hi, 20)
    assert K > 0
    b = sl.extract_traces(res, lo, hi, 20)
    assert np.array_equal(a.labels, b.labels) and a.segments.tobytes() == b.segments.tobytes()
