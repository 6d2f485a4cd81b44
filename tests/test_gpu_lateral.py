"""sl.lateral_offsets on the MI355X (sc_lateral_offsets, docs/lateral.md) against the numpy restatement
(tests/lateral_reference.py).

Integers - n, lag, lo, hi, status - match exactly: before the device is compared, the restatement's own curves are shown
to decide nothing within 1e-6 relative (the best lag against the second best, every curve value against thr), so a
difference in the last bits of a sum cannot move one, and no station is exempted.  The float fields and the mse curves
agree within 1e-9 relative - the project's figure for its float64 fits; the device and the restatement do the same
additions in the same order - with the NaNs in the same places.  Exact ties (a constant DEM), the routes, the order of
the cells and repeated runs are byte comparisons."""
import numpy as np
import pytest

import lateral_reference as lr
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, synthetic

pytestmark = pytest.mark.gpu

RTOL = 1e-9
DEMS = {"96x80": ((96, 80), 1.0, 11), "129x100": ((129, 100), 2.0, 12)}
# (h, D, q0, q1, min_samples) in cells: D = 32 makes 65 lags, a second round of the lanes; D > h at h = 3 and h = 5
PARAMS = [(3, 0, 1, 1, 3), (3, 40, 2, 9, 3), (5, 1, 2, 9, 4), (5, 31, 1, 1, 4), (5, 32, 1, 1, 4), (40, 31, 1, 1, 8),
          (40, 32, 2, 9, 8), (40, 40, 2, 9, 8)]
_Z, _REF = {}, {}


def dem(name):
    if name not in _Z:
        shape, de, seed = DEMS[name]
        _Z[name] = (lr.rough_dem(shape, seed), de)
    return _Z[name]


def stations(name, K):
    shape = DEMS[name][0]
    cells = lr.rough_stations(shape, K, 5)
    ang = np.random.default_rng(K).uniform(-np.pi, np.pi, len(cells))
    return cells, ang


def ref_of(name, K, p):
    """The restatement of a case, computed once and left unchanged."""
    key = (name, K, p)
    if key not in _REF:
        z, de = dem(name)
        cells, ang = stations(name, K)
        h, D, q0, q1, ms = p
        _REF[key] = lr.lateral_offsets(z, de, cells, ang, h, q0, q1, D, 1.0, ms)
    return _REF[key]


def run(name, K, p, cells=None, ang=None, **kw):
    z, de = dem(name)
    c0, a0 = stations(name, K)
    h, D, q0, q1, ms = p
    return sl.lateral_offsets(sl.DEMGrid.from_array(z, de), c0 if cells is None else cells, a0 if ang is None else ang,
                              h * de, q0 * de, q1 * de, D * de, min_samples=ms, **kw)


def assert_no_near_ties(rows, mse, thr):
    """On the restatement alone: at every fitted station the best and the second-best mse differ by more than 1e-6
    relative, and no curve value lies within 1e-6 relative of thr."""
    for k in np.flatnonzero(rows["status"] != 1):
        m = np.sort(mse[k][~np.isnan(mse[k])])
        assert len(m) >= 1 and m[0] == rows["mse"][k] and m[0] > 0
        if len(m) > 1:
            assert m[1] - m[0] > 1e-6 * m[0], (k, m[:2])
        assert (np.abs(m - thr[k]) > 1e-6 * thr[k]).all(), (k, thr[k])


def compare(ref, table, curve):
    rows, mse, _ = ref
    assert table.dtype.names == tuple(f for f, _ in lr.FIELDS) and len(table) == len(rows)
    for f in lr.INT_FIELDS:
        assert np.array_equal(table[f], rows[f]), (f, np.flatnonzero(table[f] != rows[f])[:5])
    worst = 0.0
    for got, want, what in [(table[f], rows[f], f) for f in lr.FLOAT_FIELDS] + [(curve, mse, "curve")]:
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok])
        assert (err <= RTOL * np.abs(want[ok])).all(), (what, err.max())
        nz = want[ok] != 0
        worst = max(worst, float((err[nz] / np.abs(want[ok][nz])).max()) if nz.any() else 0.0)
    return worst


@pytest.mark.parametrize("name", list(DEMS))
@pytest.mark.parametrize("p", PARAMS, ids=lambda p: "h%d-D%d-q%d_%d" % p[:4])
def test_against_the_restatement(name, p):
    """257 stations - not a multiple of the waves of a workgroup: the corners, cells on the borders (lags skipped,
    stations not fitted), NaN cells in the DEM, repeated cells."""
    ref = ref_of(name, 257, p)
    assert_no_near_ties(*ref)
    st = ref[0]["status"]
    table, curve = run(name, 257, p, return_curve=True)
    worst = compare(ref, table, curve)
    print("%s %r: %d of 257 fitted, %d with a lag skipped, worst relative difference %.2e"
          % (name, p, (st != 1).sum(), ((st & 16) != 0).sum(), worst))
    assert (st == 1).any() and (st != 1).sum() > 128
    if p[1] > 0:
        assert ((st & 16) != 0).any()


@pytest.mark.parametrize("K", [1, 5])
def test_few_stations(K):
    for p in (PARAMS[2], PARAMS[6]):
        ref = ref_of("96x80", K, p)
        assert_no_near_ties(*ref)
        table, curve = run("96x80", K, p, return_curve=True)
        compare(ref, table, curve)
        assert (ref[0]["status"] != 1).any()


def test_exact_ties_rank_zero_wins():
    """A constant DEM: every lag's mse is exactly 0, the first candidate wins.  Bit for bit."""
    for z, angle in ((np.zeros((96, 80)), 0.3), (np.full((96, 80), 3.0), 0.0)):
        cells = np.array([40 * 80 + 40, 50 * 80 + 30, 48 * 80 + 41, 0, 5 * 80 + 70])
        for D in (5, 40):
            rows, mse, _ = lr.lateral_offsets(z, 1.0, cells, angle, 10, 2, 6, D)
            table, curve = sl.lateral_offsets(sl.DEMGrid.from_array(z, 1.0), cells, angle, 10.0, 2.0, 6.0, float(D),
                                              return_curve=True)
            fit = table["status"] != 1
            assert fit[:3].all() and (table["lag"] == 0).all() and (table["mse"][fit] == 0.0).all()
            assert (table["lo"][:3] == -D).all() and (table["hi"][:3] == D).all() and ((table["status"][:3] & 6) == 6).all()
            assert table.tobytes() == rows.tobytes()
            assert curve.tobytes() == mse.tobytes()


def test_same_bytes_on_every_run_and_for_every_order():
    p = PARAMS[6]
    a, ac = run("129x100", 257, p, return_curve=True)
    b, bc = run("129x100", 257, p, return_curve=True)
    assert a.tobytes() == b.tobytes() and ac.tobytes() == bc.tobytes()
    assert run("129x100", 257, p).tobytes() == a.tobytes()                 # (without the curves)
    cells, ang = stations("129x100", 257)
    perm = np.random.default_rng(2).permutation(257)
    c, cc = run("129x100", 257, p, cells=cells[perm], ang=ang[perm], return_curve=True)
    assert c.tobytes() == a[perm].tobytes() and cc.tobytes() == ac[perm].tobytes()


def test_matcher_route_gives_the_same_bytes_and_leaves_the_search_alone():
    g = synthetic.synthetic_scarp(384, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    before = np.array(m.result_array())
    lo, hi = np.percentile(before[3][before[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    lab = tr.labels.ravel()[cells]
    assert len(cells) > 20 and len(tr.segments) >= 1
    # strike="segment", the default: every cell has its segment's strike from the table
    a, ac = m.lateral_offsets(tr, 30., 2., 6., 10., return_curve=True)
    assert a.dtype.names[-1] == "label" and np.array_equal(a["label"], lab) and np.array_equal(a["cell"], cells)
    assert ac.shape == (len(cells), 21)
    ang = np.asarray(tr.segments["strike"], dtype=np.float64)[lab - 1]
    b, bc = sl.lateral_offsets(g, cells, ang, 30., 2., 6., 10., return_curve=True)
    names = list(b.dtype.names)
    assert rfn(a, names).tobytes() == b.tobytes() and ac.tobytes() == bc.tobytes()
    # cells on the matcher: the result's angle plane unless told otherwise; strike="cell" reads it for the traces too
    c = m.lateral_offsets(cells, 30., 2., 6., 10.)
    d = sl.lateral_offsets(g, cells, before[2], 30., 2., 6., 10.)
    e = m.lateral_offsets(tr, 30., 2., 6., 10., strike="cell")
    assert c.tobytes() == d.tobytes() and rfn(e, names).tobytes() == d.tobytes()
    assert m.lateral_offsets(cells, 30., 2., 6., 10., angle=ang).tobytes() == b.tobytes()
    # the restatement agrees on these too
    ref = lr.lateral_offsets(np.asarray(g._griddata, dtype=np.float64), 1.0, cells, ang, 30, 2, 6, 10)
    compare(ref, b, bc)
    # the search's record and its planes are what they were
    assert np.array_equal(np.array(m.result_array()), before, equal_nan=True)


def rfn(table, names):
    """The fields ``names`` of a table as a packed array of sl.lateral_offsets' dtype."""
    from scarplet_amd import lateral
    out = np.zeros(len(table), dtype=lateral.FIT_DTYPE)
    for f in names:
        out[f] = table[f]
    return out


@pytest.mark.parametrize("theta", lr.PLANT_THETAS)
def test_the_planted_offset_on_the_device(theta):
    z = lr.planted_surface(theta)
    P = lr.PLANT
    rows = sl.lateral_offsets(sl.DEMGrid.from_array(z, 1.0), lr.planted_stations(theta), theta, float(P["h"]), float(P["q0"]),
                              float(P["q1"]), float(P["D"]))
    print(rows["lag"].tolist(), np.abs(rows["offset"] - 7.3).max(), rows["rho"].min())
    assert len(rows) == 11 and (rows["lag"] == 7).all()
    assert (np.abs(rows["offset"] - 7.3) <= 0.1).all()


def test_no_stations():
    z, de = dem("96x80")
    g = sl.DEMGrid.from_array(z, de)
    t = sl.lateral_offsets(g, [], 0.1, 10., 2., 6., 4.)
    assert len(t) == 0 and t.dtype.names == tuple(f for f, _ in lr.FIELDS)
    t, c = sl.lateral_offsets(g, np.zeros((96, 80), dtype=bool), 0.1, 10., 2., 6., 4., return_curve=True)
    assert len(t) == 0 and c.shape == (0, 9)


def test_library_refuses_what_the_header_says(gpu_ctx):
    """Every refusal comes back as an error code with a message; the context serves the next call."""
    z, de = dem("96x80")
    z = np.ascontiguousarray(z)
    cells = np.array([40 * 80 + 40], dtype=np.int64)
    sa, ca = np.sin([0.3]), np.cos([0.3])
    good = dict(h=10, q0=2, q1=6, D=4, de=1.0, delta=1.0, min_samples=8)
    bad = [dict(h=0), dict(h=1025), dict(q0=0), dict(q1=1), dict(q1=1025, q0=1000), dict(q1=66), dict(D=-1), dict(D=256),
           dict(min_samples=2), dict(min_samples=22), dict(delta=-1.0), dict(delta=np.nan), dict(de=0.0), dict(de=np.inf)]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(_lib.ScarpletHipError):
            gpu_ctx.lateral_offsets(cells, sa, ca, a["h"], a["q0"], a["q1"], a["D"], a["de"], a["delta"], a["min_samples"], z=z)
    for c, s in ((np.array([96 * 80], dtype=np.int64), sa), (np.array([-1], dtype=np.int64), sa), (cells, np.array([np.nan]))):
        with pytest.raises(_lib.ScarpletHipError):
            gpu_ctx.lateral_offsets(c, s, ca, 10, 2, 6, 4, 1.0, 1.0, 8, z=z)
    rows, _ = gpu_ctx.lateral_offsets(cells, sa, ca, 10, 2, 6, 4, 1.0, 1.0, 8, z=z)
    want = lr.lateral_offsets(z, 1.0, cells, 0.3, 10, 2, 6, 4)[0]
    assert rows["lag"][0] == want["lag"][0] and rows["status"][0] == want["status"][0]
