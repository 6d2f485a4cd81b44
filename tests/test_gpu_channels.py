"""sl.fit_channels on the MI355X (sc_channel_profiles; docs/channels.md) against the numpy restatement
(tests/channel_reference.py).

Tolerances are those of tests/test_gpu_shift.py and stand on the same ground: every compared (frequency, shift) has a
column-scaled design matrix of condition number <= 1e3 (asserted on the restatement), and the restatement agrees with a
longdouble one within 1e-11 on every input here (tests/test_channels_host.py), so sse* and the sse of the chosen pair agree
within 1e-9 relative and c0, b h de, a within 1e-9 of the profile's peak-to-peak range.  A shift d_i or an index that differs
from the restatement's must have been decided within 1e-9 relative by the restatement's own sse; cells with such a decision
may be at most 1 % of a case.  The anchors are byte comparisons.
"""
import contextlib

import numpy as np
import pytest

import channel_reference as cr
import scarplet_amd as sl
from scarplet_amd import _lib, core, synthetic

pytestmark = pytest.mark.gpu

NAMES = ["recovery 600² h100 w2 D8 F28", "de = 2, h30 w5 D4 F12", "D = h - min_samples", "D = 0", "one frequency",
         "F = 35, D = 8", "F = 64, h = 100, D = 8", "borders and corners", "NaN cells", "repeated cells", "K = 1", "no cell",
         "no live pair"]


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run(case, z=None, D=None, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_channels(grid(case["z"] if z is None else z, de), case["cells"], case["angle"], h * de, case["frequencies"],
                           swath=w * de, max_shift=(case["D"] if D is None else D) * de, delta=case["delta"],
                           min_samples=case["min_samples"], **kw)


def case_of(name):
    return cr.gpu_cases()[NAMES.index(name)]


@contextlib.contextmanager
def option(name, value, default):
    ctx = core._context(0)
    ctx.set_option(name, value)
    try:
        yield ctx
    finally:
        ctx.set_option(name, default)


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in cr.gpu_cases()] == NAMES == cr.NAMES
    for c in cr.gpu_cases():
        assert len(c["cells"]) <= 300 and 0 <= c["D"] <= min(_lib.PROFILE_MAX_SHIFT, c["h"] - c["min_samples"])


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    case = case_of(name)
    table, curve, shifts = run(case, return_curve=True, return_shift=True)
    K, F = len(case["cells"]), len(case["frequencies"])
    assert table.dtype.names[-9:] == cr.DERIVED and len(table) == K
    assert curve.shape == (K, F) and shifts.shape == (K, F) and shifts.dtype == np.int8
    nx = case["z"].shape[1]
    assert np.array_equal(table["cell"], case["cells"]) and np.array_equal(table["row"] * nx + table["col"], case["cells"])
    ref = cr.restate(case)
    st = cr.compare_rows(ref, table, curve, shifts, case["h"], case["de"], case["D"], case["delta"])
    print("%s: %s" % (name, st))
    fit = table["status"] & 1 == 0
    freqs = case["frequencies"]
    assert np.array_equal(table["f"][fit], freqs[table["f_index"][fit]])
    assert np.array_equal(table["f_lo"][fit], freqs[table["lo_index"][fit]])
    assert np.array_equal(table["f_hi"][fit], freqs[table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["f_index"][fit]], table["sse"][fit])
    assert np.abs(shifts).max(initial=0) <= case["D"]
    # what follows from f and a, by the formulas
    want = cr.derived(table["f"][fit], table["f_lo"][fit], table["f_hi"][fit], table["a"][fit])
    for f, v in want.items():
        assert np.allclose(table[f][fit], v, rtol=1e-14, atol=0), f
    assert np.all(table["width_lo"][fit] <= table["width"][fit]) and np.all(table["width"][fit] <= table["width_hi"][fit])
    sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
    assert np.array_equal(table["centre_row"][fit], (table["row"] - table["shift_index"] * sa)[fit])
    assert np.array_equal(table["centre_col"][fit], (table["col"] + table["shift_index"] * ca)[fit])
    n = np.array([r["n"] for r in ref], dtype=np.int64)
    full = n == 2 * case["h"] + 1
    if name == NAMES[0]:
        # what it is for: the device's counts are the restatement's (100 of 100; 33 of 100 without the shift)
        R = cr.REC
        assert int((table["f_index"] == R["index"]).sum()) == sum(r["f_index"] == R["index"] for r in ref) >= 95
        flat = run(case, D=0)
        zero = cr.restate(case, D=0)
        assert int((flat["f_index"] == R["index"]).sum()) == sum(r["f_index"] == R["index"] for r in zero) <= 50
        assert np.array_equal(flat["f_index"], [r["f_index"] for r in zero]) and not (table["status"] & 8).any()
    elif name == "D = 0":
        assert not (table["status"] & 8).any() and not shifts.any() and not table["shift_index"].any()
        assert np.array_equal(table["rmse"][fit], np.sqrt(table["sse"][fit] / (table["n"][fit] - 3))) and st["fitted"] == K
    elif name == "borders and corners":
        assert K % 4 and (~fit).sum() >= 4 and (fit & ~full).sum() >= 4 and (fit & full).sum() >= 15
    elif name == "NaN cells":
        assert list(n[-3:]) == [39, 39, 20] and list(table["status"][-3:] & 1) == [0, 0, 1]
        assert (fit & ~full).sum() >= 8 and (fit & full).sum() >= 8
    elif name == "no cell":
        assert K == 0
    elif name == "no live pair":
        assert list(table["status"]) == [33, 6, 6]
    else:
        assert st["fitted"] == K
    if name == "repeated cells":
        for k in range(0, K, 3):
            assert table[k:k + 3].tobytes() == table[k:k + 1].tobytes() * 3
    # a second run and the runs without the optional outputs: the same bytes
    same_bytes(run(case, return_curve=True, return_shift=True), (table, curve, shifts))
    assert run(case).tobytes() == table.tobytes()
    same_bytes(run(case, return_shift=True), (table, shifts))


# ---- bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["borders and corners", "NaN cells", "F = 35, D = 8"])
def test_a_permutation_of_the_cells_permutes_the_rows(name):
    case = case_of(name)
    perm = np.random.default_rng(5).permutation(len(case["cells"]))
    a = run(case, return_curve=True, return_shift=True)
    b = run(dict(case, cells=case["cells"][perm], angle=case["angle"][perm]), return_curve=True, return_shift=True)
    same_bytes([x[perm] for x in a], b)


@pytest.mark.parametrize("name", ["borders and corners", "NaN cells", "F = 64, h = 100, D = 8"])
def test_the_matcher_route_gives_the_same_bytes(name):
    case = case_of(name)
    h, w, de = case["h"], case["w"], case["de"]
    m = sl.Matcher(grid(case["z"], de))
    a = m.fit_channels(case["cells"], h * de, case["frequencies"], swath=w * de, max_shift=case["D"] * de, delta=case["delta"],
                       min_samples=case["min_samples"], return_curve=True, return_shift=True, angle=case["angle"])
    same_bytes(a, run(case, return_curve=True, return_shift=True))


@pytest.mark.parametrize("name", ["borders and corners", "NaN cells", "F = 35, D = 8"])
def test_chunks_of_three_cells_give_the_bytes_of_one_chunk(name):
    case = case_of(name)
    one = run(case, return_curve=True, return_shift=True)
    with option("fit_chunk", 3, 0) as ctx:
        ctx.profile(1)
        n0 = ctx.profile_get()["k_profile"][0]
        many = run(case, return_curve=True, return_shift=True)
        launches = ctx.profile_get()["k_profile"][0] - n0
        ctx.profile(0)
    same_bytes(many, one)
    assert launches == 2 + -(-len(case["cells"]) // 3)                     # the table, the terms, a launch per chunk


@pytest.mark.parametrize("name", ["borders and corners", "NaN cells", "F = 35, D = 8", "F = 64, h = 100, D = 8", "one frequency"])
def test_the_terms_table_changes_no_byte(name):
    """A complete profile takes ebar, gamma and See of a pair from the table of the call ("channel_terms" 1) or sweeps for them
    ("channel_terms" 0): the same operations in the same order, the same bytes in the rows, the curves and the shift planes.
    The borders case and the NaN case hold complete and clipped profiles in one workgroup: both routes run in one launch."""
    case = case_of(name)
    n = np.array([r["n"] for r in cr.restate(case)])
    assert (n == 2 * case["h"] + 1).sum() >= 8
    fast = run(case, return_curve=True, return_shift=True)
    with option("channel_terms", 0, 1):
        slow = run(case, return_curve=True, return_shift=True)
    same_bytes(fast, slow)
    assert (fast[0]["status"] & 1 == 0).sum() >= 8


# ---- exact anchors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F = 35, D = 8", "borders and corners", "NaN cells"])
def test_the_fit_of_the_negated_surface(name):
    """Negation commutes with rounding: fit(-z) has the indices, the shifts and the sse of fit(z), and a, b, c0 negated."""
    case = case_of(name)
    t, c, s = run(case, return_curve=True, return_shift=True)
    u, d, v = run(case, z=-case["z"], return_curve=True, return_shift=True)
    for f in ("n", "f_index", "lo_index", "hi_index", "status", "shift_index", "sse", "rmse", "f", "shift"):
        assert t[f].tobytes() == u[f].tobytes(), f
    assert c.tobytes() == d.tobytes() and s.tobytes() == v.tobytes()
    fit = t["status"] & 1 == 0
    assert fit.sum() >= 8
    for f in ("a", "b", "c0"):
        assert (-t[f][fit]).tobytes() == u[f][fit].tobytes(), f
    assert np.array_equal(t["depth"][fit], -u["depth"][fit]) and np.array_equal(t["curvature"][fit], -u["curvature"][fit])


def test_a_cell_off_the_thalweg_returns_minus_its_offset():
    """A noise-free trough along column 60 at orientation 0: the profile runs along +col, so a cell k columns off the thalweg
    has the trough's centre at d = -k, and centre_col is the thalweg's column.  This pins the sign of the shift."""
    f0 = float(cr.freqs_of_sigma([4.0])[0])
    c = np.arange(128, dtype=np.float64) - 60.0
    z = np.repeat((-np.exp(-(np.pi * f0 * c) ** 2) + 0.01 * c)[None, :], 96, axis=0)
    k = np.arange(-5, 6)
    t = sl.fit_channels(grid(z, 1.0), 48 * 128 + 60 + k, 0.0, 30.0, f0 * 1.12 ** np.arange(-5, 6), swath=1.0, max_shift=8.0)
    assert np.array_equal(t["shift_index"], -k) and np.array_equal(t["centre_col"], np.full(11, 60.0))
    assert np.array_equal(t["centre_row"], np.full(11, 48.0)) and (t["f_index"] == 5).all() and (t["status"] == 0).all()
    assert np.abs(t["depth"] - 1.0).max() <= 1e-9 and np.abs(t["b"] - 0.01).max() <= 1e-9


# ---- against the search --------------------------------------------------------------------------------------------------
def test_the_search_and_the_fit_agree_on_sign_and_scale():
    """docs/channels.md, "Against the search": Matcher.search(Channel) at the trough's own frequency, extract_traces, and
    Matcher.fit_channels on the largest segment.  On the CPU the oracle and the restatement give amp > 0 and a < 0 in every
    cell and a median amp / curvature of 0.9856 (tests/test_channels_host.py) over the cells 100 and more from every border,
    where the search's window and the profile are complete; the device is allowed one percentage point under that share and
    2 % around that median - what float32 amplitudes against float64 fits leave."""
    S = cr.SEARCH
    m = sl.Matcher(synthetic.synthetic_channel(S["n"]))
    m.search(sl.Channel, S["scale"], [S["f0"]], np.linspace(-S["ang"], S["ang"], 35))
    res = np.array(m.result_array())
    top = float(np.nanmax(res[3]))
    tr = m.extract_traces(0.25 * top, 0.5 * top, 4)
    seg = tr.segments
    label = int(seg["label"][np.argmax(seg["n_cells"])])
    t = m.fit_channels(tr, float(S["h"]), cr.search_frequencies(), swath=float(S["w"]), max_shift=float(S["D"]))
    assert t.dtype.names[-1] == "label" and np.array_equal(t["label"], tr.labels.ravel()[t["cell"]])
    lo, hi = S["margin"], S["n"] - S["margin"]
    t = t[(t["label"] == label) & (t["row"] >= lo) & (t["row"] < hi) & (t["col"] >= lo) & (t["col"] < hi)]
    assert len(t) >= 250 and (t["status"] & 1 == 0).all()
    amp = res[0].ravel()[t["cell"]]
    share = float(((amp > 0) & (t["a"] < 0)).mean())
    ratio = float(np.median(amp / t["curvature"]))
    print("%d cells of segment %d: amp > 0 and a < 0 in %.4f of them, median amp / curvature %.4f" % (len(t), label, share, ratio))
    assert share >= cr.SEARCH_SHARE - 0.01
    assert abs(ratio / cr.SEARCH_RATIO - 1.0) <= 0.02
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)


def test_library_refuses_what_the_header_says():
    ctx = _lib.Context(0)
    z = cr.channel_z(64)
    f = np.array([0.05, 0.1])
    cells, sa, ca = np.array([5 * 64 + 30, 6 * 64 + 30], dtype=np.int64), np.zeros(2), np.ones(2)

    def call(D=2, h=10, ms=4, freqs=f, de=1.0):
        return ctx.channel_profiles(cells, sa, ca, np.asarray(freqs, dtype=np.float64), h, 1, D, de, 1.0, ms, z=z)
    assert (call(6)[0]["status"] & 1 == 0).all()                           # D = h - min_samples is the last one taken
    assert (call(freqs=[6.0 / np.pi])[0]["status"] & 1 == 0).all()         # pi f de = 6 too
    for kw in (dict(D=-1), dict(D=7), dict(D=5, ms=6), dict(freqs=[0.1, 0.05]), dict(freqs=[0.0, 0.05]), dict(freqs=[0.05, np.nan]),
               dict(freqs=[0.05, 2.0]), dict(freqs=[0.05, 1.0], de=2.0)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            call(**kw)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        call(65, h=100)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        call(freqs=np.linspace(0.01, 0.1, 65))
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        ctx.channel_profiles(cells, sa, ca, f, 10, 1, 2, 1.0, 1.0, 4)       # no DEM set
    for bad in (2, -1, 0.5, np.nan):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\).*channel_terms"):
            ctx.set_option("channel_terms", bad)
    ctx.close()
