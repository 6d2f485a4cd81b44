"""sl.snr_surface on the device against the float64 oracle and the numpy restatement (tests/surface_reference.py).

The cases (surface_reference.cases) score ALL cells of small DEMs: corners and edges (the reference's transform is circular),
the window-limit border where every template is masked (status 1), grids of three ages on four waves, de = 2 and dy < 0, an
UpperBreak's error mask, a Ricker, runs longer than a wave with five ages and several row groups (F), and an 8 x 12 grid
whose intervals are wider than one index (E).  Tolerance of the cubes: 1e-9 of the template's largest oracle value over the
map, the existing float64 scorer's own (test_float64_scoring_of_single_cells).  The argmax is compared where the oracle's two
top scores differ by more than 2e-9 M (twice that tolerance; test_surface_host.py counts the cells this excludes)."""
import numpy as np
import pytest

import surface_reference as ref
import scarplet_amd as sl
from scarplet_amd import _lib

pytestmark = pytest.mark.gpu

CB = _lib.SURFACE_CELL_BATCH
_RUNS = {}


def grid(c):
    return sl.DEMGrid.from_array(c["z"], float(c["de"]), float(c["dy"]))


def matcher(gpu_ctx, name):
    return sl.Matcher(grid(ref.cases()[name]), ctx=gpu_ctx)


def run(gpu_ctx, name, drop=0.1):
    """(table, S, Amp) of case ``name`` at all its cells - one device call per (case, drop), shared by the tests."""
    key = (name, drop)
    if key not in _RUNS:
        c = ref.cases()[name]
        m = matcher(gpu_ctx, name)
        out = m.snr_surface(getattr(sl, c["cls"]), c["scale"], c["params"], c["angles"], np.arange(c["z"].size), drop=drop,
                            return_surface=True)
        for v in out:
            v.setflags(write=False)
        _RUNS[key] = out
    return _RUNS[key]


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "F", "E"])
def test_cube_and_argmax_against_the_oracle(gpu_ctx, name):
    tab, S, Amp = run(gpu_ctx, name)
    oS, oA, smax, amax = ref.oracle_cubes(name)
    assert S.shape == oS.shape and Amp.shape == oA.shape and S.dtype == np.float64
    es = (np.abs(S - oS).max(axis=0) / np.maximum(smax, 1e-300)).max()
    ea = (np.abs(Amp - oA).max(axis=0) / np.maximum(amax, 1e-300)).max()
    live, excluded, (ia, ib) = ref.oracle_ties(name)
    print("case %s: %d cells, %d live, %d excluded; snr error %.2e, amp error %.2e of the template's largest"
          % (name, len(tab), live.sum(), excluded.sum(), es, ea))
    assert es <= 1e-9 and ea <= 1e-9, (name, es, ea)
    assert excluded.sum() <= 1e-3 * live.sum()
    ok = live & ~excluded
    assert np.array_equal(tab["par_index"][ok], ia[ok]) and np.array_equal(tab["ang_index"][ok], ib[ok])
    assert np.array_equal(tab["status"] == 1, ~live) and ((~live).any() or name == "D")      # (a Ricker has no window limits)
    dead = tab[~live]
    assert (dead["par_index"] == -1).all() and (dead["n_within"] == 0).all() and np.isnan(dead["snr"]).all() \
        and np.isnan(dead["par"]).all() and np.isnan(dead["angle_hi"]).all()
    c = ref.cases()[name]
    assert np.array_equal(tab["cell"], np.arange(len(tab))) and np.array_equal(tab["row"], tab["cell"] // c["z"].shape[1])
    assert np.array_equal(tab["par"][live], c["params"][tab["par_index"][live]])
    assert np.array_equal(tab["angle_lo"][live], c["angles"][tab["ang_lo_index"][live]])


@pytest.mark.parametrize("name,drop", [("A", 0.1), ("F", 0.1), ("E", 0.1), ("E", 0.5), ("E", 0.0)])
def test_the_table_is_the_restatement_of_the_cube(gpu_ctx, name, drop):
    tab, S, Amp = run(gpu_ctx, name, drop)
    want = ref.reduce_cube(S, Amp, drop)
    got = ref.table_rows(tab)
    for f in want.dtype.names:
        assert same_bytes(got[f], want[f]), (name, drop, f, np.flatnonzero(got[f].view(np.int64 if f in ("snr", "amp") else np.int32)
                                                                          != want[f].view(np.int64 if f in ("snr", "amp") else np.int32))[:5])
    if name == "E" and drop == 0.5:
        live = tab["status"] != 1
        assert ((tab["par_hi_index"] - tab["par_lo_index"])[live] > 1).any() and ((tab["ang_hi_index"] - tab["ang_lo_index"])[live] > 1).any()
        st = tab["status"][live]
        assert all((st & b).any() for b in (2, 4, 8, 16)) and (st & 6 == 6).any()
    if drop == 0.0:
        assert (tab["n_within"][tab["status"] != 1] >= 1).all()


def test_batches_and_degenerate_grids(gpu_ctx):
    c = ref.cases()["E"]
    tab, S, Amp = run(gpu_ctx, "E")
    m = matcher(gpu_ctx, "E")
    nx = c["z"].shape[1]
    call = lambda cells, par=c["params"], ang=c["angles"]: m.snr_surface(sl.Scarp, c["scale"], par, ang, cells, return_surface=True)
    first = 40 * nx + 30
    for K in (1, CB - 1, CB, CB + 1):
        cells = np.arange(first + 3, first + 3 + K)                          # (batches that do not line up with the all-cells run's)
        t, s, a = call(cells)
        assert same_bytes(t, tab[cells]) and same_bytes(s, S[cells]) and same_bytes(a, Amp[cells]), K
    rng = np.random.default_rng(5)
    cells = rng.integers(0, c["z"].size, 257)
    cells[200:] = cells[:57]                                               # repeats
    cells = rng.permutation(cells)
    t, s, a = call((cells // nx, cells % nx))                              # (the (rows, cols) form)
    assert same_bytes(t, tab[cells]) and same_bytes(s, S[cells]) and same_bytes(a, Amp[cells])
    # one orientation, one age: their own union boxes - against the oracle and the restatement
    oS, oA, smax, amax = ref.oracle_cubes("E")
    allc = np.arange(c["z"].size)
    for par, ang, sel in ((c["params"], c["angles"][4:5], (slice(None), slice(4, 5))),
                          (c["params"][3:4], c["angles"], (slice(3, 4), slice(None)))):
        t, s, a = call(allc, par, ang)
        assert s.shape == (len(allc), len(par), len(ang))
        o = oS[(slice(None),) + sel]
        assert (np.abs(s - o).max(axis=0) / smax[sel]).max() <= 1e-9
        assert (np.abs(a - oA[(slice(None),) + sel]).max(axis=0) / amax[sel]).max() <= 1e-9
        want = ref.reduce_cube(s, a, 0.1)
        got = ref.table_rows(t)
        assert all(same_bytes(got[f], want[f]) for f in want.dtype.names)
        livec = t["status"] != 1
        if len(par) == 1:
            assert (t["status"][livec] & 6 == 6).all()
        else:
            assert (t["status"][livec] & 24 == 24).all()


def test_the_scorers_last_search_is_the_surfaces_table(gpu_ctx):
    """ctx.score_cells_f64 after snr_surface scores the surface's templates with their own n and sum(W**2): in a context that
    never searched, and in one whose last search held another number of templates and other windows."""
    c = ref.cases()["A"]
    tab, S, Amp = run(gpu_ctx, "A")
    oS, oA, smax, amax = ref.oracle_cubes("A")
    ny, nx = c["z"].shape
    cells = np.arange(0, ny * nx, 7)
    rc = np.column_stack(np.divmod(cells, nx)).astype(np.int32)
    n_par, n_ang = len(c["params"]), len(c["angles"])
    fresh = _lib.Context(0)
    try:
        for ctx, before in ((fresh, None), (gpu_ctx, ([2.0, 9.0, 30.0, 70.0], [-0.4, 0.3]))):
            m = sl.Matcher(grid(c), ctx=ctx)
            if before:
                m.search(sl.Scarp, 5, before[0], before[1], method="direct")
            t, s, a = m.snr_surface(sl.Scarp, c["scale"], c["params"], c["angles"], cells, return_surface=True)
            assert same_bytes(s, S[cells]) and same_bytes(t, tab[cells])
            amp, snr = ctx.score_cells_f64(rc, n_par * n_ang)
            snr = snr.reshape(-1, n_ang, n_par).transpose(0, 2, 1)
            amp = amp.reshape(-1, n_ang, n_par).transpose(0, 2, 1)
            assert (np.abs(snr - oS[cells]).max(axis=0) / smax).max() <= 1e-9
            assert (np.abs(amp - oA[cells]).max(axis=0) / amax).max() <= 1e-9
            with pytest.raises(_lib.ScarpletHipError, match="expects"):
                ctx.score_cells_f64(rc, n_par * n_ang + 1)
    finally:
        fresh.close()


def test_two_calls_return_the_same_bytes(gpu_ctx):
    c = ref.cases()["F"]
    first = run(gpu_ctx, "F")
    again = matcher(gpu_ctx, "F").snr_surface(sl.Scarp, c["scale"], c["params"], c["angles"], np.arange(c["z"].size),
                                               return_surface=True)
    assert all(same_bytes(x, y) for x, y in zip(first, again))


_RNG = np.random.default_rng(20261019)
_BASE = _RNG.standard_normal((9, 11))
_BASE[_RNG.random((9, 11)) < 0.2] = 0.0                # a support with holes


class Plugin(object):
    """No _device_descriptor: template() and the masks are uploaded.  Its alpha is not the orientation."""

    def __init__(self, d, age, angle, nx, ny, de):
        self.age, self.angle, self.nx, self.ny = age, angle, nx, ny
        self.alpha = 0.3 - angle

    def template(self):
        W = np.zeros((self.ny, self.nx))
        cy, cx = self.ny // 2, self.nx // 2
        W[cy - 4:cy + 5, cx - 5:cx + 6] = _BASE * (1.0 + 0.1 * self.age * np.linspace(-1, 1, 11)[None, :])
        return W

    def get_window_limits(self):
        lim = np.random.default_rng(3).random((self.ny, self.nx)) < 0.03
        lim[:6, :] = lim[-5:, :] = True
        lim[:, :7] = lim[:, -6:] = True
        return lim

    def get_err_mask(self):
        return np.random.default_rng(5000 + int(round(1000 * self.angle))).random((self.ny, self.nx)) < 0.05


def test_a_plugin_with_uploaded_windows(gpu_ctx):
    c = ref.cases()["A"]
    m = matcher(gpu_ctx, "A")
    ages, angles = np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([-1.0, -0.2, 0.6, 1.3])
    ny, nx = c["z"].shape
    try:
        m.search(Plugin, 10, ages, angles, method="direct", exact=False)
        rc = np.column_stack(np.divmod(np.arange(ny * nx), nx)).astype(np.int32)
        amp, snr = m.ctx.score_cells_f64(rc, len(ages) * len(angles))
        tab, S, Amp = m.snr_surface(Plugin, 10, ages, angles, np.arange(ny * nx), return_surface=True)
    finally:
        gpu_ctx.clear_windows()
    old_s = snr.reshape(-1, len(angles), len(ages)).transpose(0, 2, 1)      # hand-over order: orientation-major
    old_a = amp.reshape(-1, len(angles), len(ages)).transpose(0, 2, 1)
    es = (np.abs(S - old_s).max(axis=0) / old_s.max(axis=0)).max()
    ea = (np.abs(Amp - old_a).max(axis=0) / np.abs(old_a).max(axis=0)).max()
    print("plugin: snr %.2e, amp %.2e" % (es, ea))
    assert es <= 1e-9 and ea <= 1e-9
    assert (S == 0).any() and (tab["status"] == 1).any() and (tab["status"] != 1).any()
    got, want = ref.table_rows(tab), ref.reduce_cube(S, Amp, 0.1)
    assert all(same_bytes(got[f], want[f]) for f in want.dtype.names)


def test_the_exact_search_carries_the_table(gpu_ctx):
    c = ref.cases()["E"]
    tab = run(gpu_ctx, "E")[0]
    m = matcher(gpu_ctx, "E")
    before = m.search(sl.Scarp, c["scale"], c["params"], c["angles"], exact=True).result_array().copy()
    live = tab["status"] != 1
    assert np.array_equal(before[1].ravel()[live], tab["par"][live]) and np.array_equal(before[2].ravel()[live], tab["angle"][live])
    # the routes: the Matcher's call leaves the record alone and returns sl.snr_surface's bytes; Traces give the label column
    tr = m.extract_traces(float(np.percentile(before[3], 90)))
    t2 = m.snr_surface(sl.Scarp, c["scale"], c["params"], c["angles"], tr)
    assert same_bytes(m.result_array(), before)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) and np.array_equal(t2["cell"], cells) and np.array_equal(t2["label"], tr.labels.ravel()[cells])
    assert t2.dtype.names == tab.dtype.names + ("label",) and all(same_bytes(t2[f], tab[cells][f]) for f in tab.dtype.names)
    top = sl.snr_surface(grid(c), sl.Scarp, np.arange(c["z"].size), c["scale"], ages=c["params"], angles=c["angles"],
                         return_surface=True)
    assert all(same_bytes(x, y) for x, y in zip(top, run(gpu_ctx, "E")))
