"""The initial slope of sl.fit_profiles on the MI355X (sc_fit_profiles_ramp; docs/profiles.md "The initial slope") against
the numpy restatement (tests/ramp_reference.py).

Tolerances are those of tests/test_gpu_profiles.py and stand on the same ground: every compared (age, half-width) has a
column-scaled design matrix of condition number <= 1e3, and the age grids of the cases are cut further, to where the
float64 restatement and its longdouble twin agree within 1e-11 (tests/test_ramp_host.py: the column of a ramp is a
difference of two table entries, whose rounding the fit amplifies more than the erf's) - so sse* and the sse of the chosen
pair agree within 1e-9 relative and c0, b h de, a within 1e-9 of the profile's peak-to-peak range.  An m_i or an index
that differs from the restatement's must have been decided within 1e-9 relative by the restatement's own key; cells with
such a decision may be at most 1 % of a case.  The anchors are byte comparisons.
"""
import numpy as np
import pytest

import profile_reference as pr
import ramp_reference as rr
import scarplet_amd as sl
from scarplet_amd import _lib

pytestmark = pytest.mark.gpu


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run(case, mode=rr.FREE, M="case", **kw):
    h, w, de = case["h"], case["w"], case["de"]
    M = case["M"] if M == "case" else M
    if mode == rr.SLOPE:
        kw["initial_slope"] = case["slope"]
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], max_width=None if M is None else M * de, **kw)


CASES = None


def case_of(name):
    global CASES
    if CASES is None:
        CASES = {c["name"]: c for c in rr.gpu_cases()}
    return CASES[name]


MODES = {"free": rr.FREE, "slope": rr.SLOPE}
# (the case of the cell with dof < 1 is about the free width: with the slope given that cell has a degree of freedom)
PARAMS = [(n, m) for n in rr.NAMES for m in MODES if not (n == "dof < 1" and m == "slope")]


@pytest.mark.parametrize("name,mode", PARAMS)
def test_profiles_against_the_restatement(name, mode):
    case, md = case_of(name), MODES[mode]
    table, curve, widths = run(case, md, return_curve=True, return_width=True)
    K, A, M = len(case["cells"]), len(case["ages"]), case["M"]
    assert table.dtype.names[-3:] == ("width_index", "width", "initial_slope") and len(table) == K
    assert curve.shape == (K, A) and widths.shape == (K, A) and widths.dtype == np.int8
    nx = case["z"].shape[1]
    assert np.array_equal(table["cell"], case["cells"]) and np.array_equal(table["row"] * nx + table["col"], case["cells"])
    ref = rr.restate(case, md)
    st = rr.compare_rows(ref, table, curve, widths, case["h"], case["de"], M, md, case["slope"], case["delta"])
    print("%s, %s: %s" % (name, mode, st))
    fit = table["status"] != 1
    assert np.array_equal(table["kt"][fit], case["ages"][table["kt_index"][fit]])
    assert np.array_equal(table["kt_lo"][fit], case["ages"][table["lo_index"][fit]])
    assert np.array_equal(table["kt_hi"][fit], case["ages"][table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["sse"][fit])
    n = np.array([r["n"] for r in ref], dtype=np.int64)
    dof = n - 3 - (1 if md == rr.FREE and M > 0 else 0)
    assert np.array_equal(table["rmse"][fit], np.sqrt(table["sse"][fit] / dof[fit]))
    if name == "no cell":
        assert K == 0
    elif name in ("borders and corners", "NaN cells"):
        assert (~fit).sum() > 0 or name == "NaN cells"
        assert (fit & (n < 2 * case["h"] + 1)).sum() >= 5                   # fitted with points missing
    elif name == "dof < 1":
        assert list(table["status"] & 1) == [1, 0, 0, 0] and list(table["n"]) == [4, 7, 7, 7]
    else:
        assert st["fitted"] == K
    if name == "repeated cells":
        for k in range(0, K, 3):
            assert table[k:k + 3].tobytes() == table[k:k + 1].tobytes() * 3
    # a second run and the runs without the optional outputs: the same bytes
    t2, c2, w2 = run(case, md, return_curve=True, return_width=True)
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == curve.tobytes() and w2.tobytes() == widths.tobytes()
    assert run(case, md).tobytes() == table.tobytes()
    t3, w3 = run(case, md, return_width=True)
    assert t3.tobytes() == table.tobytes() and w3.tobytes() == widths.tobytes()


SHARED = [f for f in _lib.PROFILE_DTYPE.names] + ["row", "col", "height"]


@pytest.mark.parametrize("name", ["h100 w0 M8", "64 ages M1", "borders and corners", "NaN cells", "de 2"])
def test_width_zero_is_the_plain_call_byte_for_byte(name):
    """max_width=0 goes through k_pf_ramp and returns the bytes of sc_fit_profiles in every shared field."""
    case = case_of(name)
    plain, pc = run(case, M=None, return_curve=True)
    zero, zc, zw = run(case, M=0, return_curve=True, return_width=True)
    assert "width" not in plain.dtype.names and len(zero) == len(plain) > 0
    for f in SHARED:
        assert zero[f].tobytes() == plain[f].tobytes(), f
    assert zc.tobytes() == pc.tobytes() and not zw.any()
    fit = plain["status"] != 1
    assert fit.any() and not zero["width_index"].any()
    assert np.array_equal(zero["width"][fit], np.zeros(fit.sum())) and np.isnan(zero["width"][~fit]).all()
    assert np.array_equal(zero["initial_slope"][fit], np.copysign(np.inf, plain["a"][fit]))
    assert np.isnan(zero["initial_slope"][~fit]).all()
    assert not (zero["status"] & 8).any()


@pytest.mark.parametrize("mode", list(MODES))
def test_a_permutation_of_the_cells_permutes_the_rows(mode):
    case = case_of("borders and corners")
    table, curve, widths = run(case, MODES[mode], return_curve=True, return_width=True)
    perm = np.random.default_rng(8).permutation(len(case["cells"]))
    shuffled = dict(case, cells=case["cells"][perm], angle=case["angle"][perm])
    t2, c2, w2 = run(shuffled, MODES[mode], return_curve=True, return_width=True)
    assert t2.tobytes() == table[perm].tobytes()
    assert c2.tobytes() == curve[perm].tobytes() and w2.tobytes() == widths[perm].tobytes()


def test_matcher_route_gives_the_same_bytes():
    """Matcher.fit_profiles(traces, ...) on the DEM it holds against sl.fit_profiles on the same cells."""
    from scarplet_amd import traces
    case = case_of("h30 w5 M4")
    g = grid(case["z"], 1.0)
    ny, nx = case["z"].shape
    m = sl.Matcher(g)
    labels = np.zeros((ny, nx), dtype=np.int32)
    cells = np.unique(case["cells"])
    labels.ravel()[cells] = 1 + np.arange(len(cells)) % 3
    tr = traces.Traces(labels > 0, labels, traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(max_width=4.0), dict(max_width=4.0, initial_slope=0.3)):
        a, ac, aw = m.fit_profiles(tr, 30.0, swath=5.0, ages=case["ages"], min_samples=15, angle=0.2, return_curve=True,
                                   return_width=True, **kw)
        b, bc, bw = sl.fit_profiles(g, cells, 0.2, 30.0, swath=5.0, ages=case["ages"], min_samples=15, return_curve=True,
                                    return_width=True, **kw)
        assert a.dtype.names == b.dtype.names + ("label",) and np.array_equal(a["label"], labels.ravel()[cells])
        for f in b.dtype.names:
            assert a[f].tobytes() == b[f].tobytes(), f
        assert ac.tobytes() == bc.tobytes() and aw.tobytes() == bw.tobytes() and (b["status"] != 1).all()
        c = m.fit_profiles(cells, 30.0, swath=5.0, ages=case["ages"], min_samples=15, angle=0.2, **kw)
        assert c.tobytes() == b.tobytes()


def test_recovery_counts_are_the_restatements():
    """The recovery surface of docs/profiles.md: the device's counts equal the restatement's - the true age in at least 90
    of the 100 cells with the slope given and in at most 10 with the plain call; without noise and with the width free,
    width_index 6 and index 10 in every cell."""
    R = rr.REC
    z, cells, theta, ages = rr.recovery_case()
    pairs = rr.pairs_of_cells(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages)
    ref = rr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages, mode=rr.SLOPE, slope=R["slope"], pairs=pairs)
    g = grid(z, 1.0)
    given = sl.fit_profiles(g, cells, theta, R["h"], swath=R["w"], ages=ages, max_width=R["M"], initial_slope=R["slope"])
    plain = sl.fit_profiles(g, cells, theta, R["h"], swath=R["w"], ages=ages)
    hit, miss = int((given["kt_index"] == R["index"]).sum()), int((plain["kt_index"] == R["index"]).sum())
    print("true age: %d of 100 with the slope given, %d with the plain call" % (hit, miss))
    assert hit == sum(r["kt_index"] == R["index"] for r in ref)
    assert miss == sum(r["kt_index"] == R["index"] for r in pr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], ages))
    assert hit >= 90 and miss <= 10
    free_ref = rr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages, pairs=pairs)
    free = sl.fit_profiles(g, cells, theta, R["h"], swath=R["w"], ages=ages, max_width=R["M"])
    assert int((free["kt_index"] == R["index"]).sum()) == sum(r["kt_index"] == R["index"] for r in free_ref)
    z0 = rr.recovery_case(0.0)[0]
    clean = sl.fit_profiles(grid(z0, 1.0), cells, theta, R["h"], swath=R["w"], ages=ages, max_width=R["M"])
    assert (clean["width_index"] == R["L"]).all() and (clean["kt_index"] == R["index"]).all() and (clean["status"] == 0).all()


def test_a_ramp_wider_than_the_range_sets_status_8():
    """A planted half-width of 6 cells with max_width 3, on an age grid that ends at the true age: the best age's m is the
    end of the range, and the row says so.  (On the whole grid an older age takes up the missing width - kt + L^2 / 6,
    docs/profiles.md - and the row is index 12 with m = 2, unflagged: the restatement's answer, and the device's.)"""
    R = rr.REC
    z, cells, theta, ages = rr.recovery_case(0.0)
    g = grid(z, 1.0)
    t = sl.fit_profiles(g, cells, theta, R["h"], swath=R["w"], ages=ages[:R["index"] + 1], max_width=3.0)
    assert (t["width_index"] == 3).all() and (t["status"] & 8 == 8).all() and (t["width"] == 3.0).all()
    assert (t["kt_index"] == R["index"]).all() and (t["status"] == 8 + 4).all()
    wide = sl.fit_profiles(g, cells, theta, R["h"], swath=R["w"], ages=ages, max_width=8.0)
    assert not (wide["status"] & 8).any()
    whole = sl.fit_profiles(g, cells, theta, R["h"], swath=R["w"], ages=ages, max_width=3.0)
    assert (whole["kt_index"] == 12).all() and (whole["width_index"] == 2).all() and not (whole["status"] & 8).any()


def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = rr.ramp_scarp(64, 1.0, 1.0, theta=0.0, noise=0.01, seed=3)
    ages = np.array([1.0, 2.0])
    cells, sa, ca = np.array([5 * 64 + 30, 6 * 64 + 30], dtype=np.int64), np.zeros(2), np.ones(2)

    def call(M, mode=_lib.RAMP_FREE, slope=0.0, h=10, ms=4):
        return ctx.fit_profiles_ramp(cells, sa, ca, ages, h, 1, 1.0, 1.0, ms, M, mode=mode, slope=slope, z=z)
    assert (call(6)[0]["status"] & 1 == 0).all()                           # M = h - min_samples is the last one taken
    assert (call(6, _lib.RAMP_SLOPE, 0.5)[0]["status"] & 1 == 0).all()
    for kw in (dict(M=-1), dict(M=7), dict(M=5, ms=6), dict(M=4, mode=2), dict(M=4, mode=-1), dict(M=0, mode=_lib.RAMP_SLOPE, slope=0.5),
               dict(M=4, mode=_lib.RAMP_SLOPE, slope=0.0), dict(M=4, mode=_lib.RAMP_SLOPE, slope=-0.5),
               dict(M=4, mode=_lib.RAMP_SLOPE, slope=np.inf), dict(M=4, mode=_lib.RAMP_SLOPE, slope=np.nan)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            call(**kw)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        call(65, h=100)
    assert (call(4, _lib.RAMP_FREE, np.nan)[0]["status"] & 1 == 0).all()    # the slope is read with SC_RAMP_SLOPE alone
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        ctx.fit_profiles_ramp(cells, sa, ca, ages, 10, 1, 1.0, 1.0, 4, 2)   # no DEM set
    ctx.close()
