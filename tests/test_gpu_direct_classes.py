"""Every kernel class of the real-space path against the float64 oracle, and the classes against each other bit for bit.

direct_route (scarplet_amd/csrc/sc_direct_route.h) sends a launch to one of eight instantiations k_direct2<NB, RW, SHARE,
W4> by the DEM's size and the launch's window box; match_impl folds up to 32 orientations in one launch on small DEMs;
the kernel stages a template in as many slabs as the LDS asks for.  The suite's other real-space tests run on DEMs of at
most 750 000 cells - the 256 x 8 class only.  tests/direct_classes.py names, case by case, the DEM, the template family,
the parameters and the option that reach each class, batch regime and slab count, and tests/test_direct_route_host.py
holds every case to its name on the CPU with the route's own functions; here the cases run.

(a) test_class_against_oracle: a fold (sc_match, float32 mode) and one template's maps (sc_match_template) of every case.
    The small DEMs are checked over the whole grid (orc.snr_stack); the large ones over every cell of a dozen windows
    (orc.snr_stack_window on crops of the periodic DEM: margin = the templates' reach plus the stencil, the crop keeps
    the DEM's parity) placed where a class's indexing can break - the four corners (the slab wraps on both axes), astride
    the patch seams in x (256 k: a 512 patch's seam or its +256 block) and in y (16 k and 16 k + 8), in the partial last
    patch on either axis, astride the window-limit border, and one in the interior.
(b) test_uploaded_window_against_oracle: host-uploaded windows (orc.match_arrays on the whole DEM) - the run-length window,
    whose rows are single runs of SC_DR_SHARE_MIN - 4 .. + 8 taps at every start offset within a group of four, with and
    without a hole, in an order that meets every transition of the kernel's look-ahead; and tall windows staged in
    several slabs.
(c) test_classes_agree_bit_for_bit: the slab's size "decides only how many template rows are staged at a time, not the
    order of any sum" (sc_direct_route.h) - one search through two classes, two slab counts or two batch regimes leaves
    the same record and the same maps in every bit; with option "near_window" on, the same record again and the same
    flagged cells.  A rank's sub-rectangle of a sharded DEM may take another class than the whole DEM: this is why the
    shards' records fit together.

The tolerances are the project's own (oracle.PARITY, snr_tolerance, tie_window("direct")) and the policy is report()'s:
no cell outside the tolerances, no cell off the oracle's argmax, the measured SNR error at most half the tie window.
Every case prints one line in report()'s format (pytest -s); profiles/direct_classes.txt holds those lines as measured,
with the build id of the library that gave them."""
import numpy as np
import pytest

import scarplet_oracle as orc
import scarplet_amd as sl
from scarplet_amd import WindowedTemplate as WT
from scarplet_amd.core import _near_window
from parity_report import report
import direct_classes as dc

pytestmark = pytest.mark.gpu

P_AMP = orc.PARITY["amp"]


def matcher(gpu_ctx, name):
    return sl.Matcher(dc.dem(name), ctx=gpu_ctx)


class options(object):
    """The case's options "variant" and "batch" for the searches inside; both back at their defaults on the way out."""

    def __init__(self, ctx, c):
        self.ctx, self.c = ctx, c

    def __enter__(self):
        self.ctx.set_option("variant", self.c["variant"])
        self.ctx.set_option("batch", 0 if self.c["batch_off"] else 1)

    def __exit__(self, *exc):
        self.ctx.set_option("variant", 0)
        self.ctx.set_option("batch", 1)


def described(m, c):
    """The case's descriptors and plan; the boxes are the table's (what the host test routed)."""
    arr, bbox, max_area = m.describe(dc.FAMILIES[c["family"]][0], c["scale"], np.asarray(c["params"], float), np.asarray(c["angles"], float))
    assert tuple(bbox) == dc.boxes(c)[2], (c["name"], bbox)
    wh, ww, _ = dc.boxes(c)
    n_ang = len(c["angles"])
    for k in range(len(arr)):                      # (descriptor k: angle k // n_par, parameter k % n_par; id = ia * n_ang + ib)
        ib, ia = divmod(k, len(c["params"]))
        assert arr[k].id == ia * n_ang + ib
        assert (arr[k].pmax - arr[k].pmin + 1, arr[k].qmax - arr[k].qmin + 1) == (wh[ib, ia], ww[ib, ia]), (c["name"], k)
    _, sp = m.plan_for(bbox, max_area, "direct", None, n_params=len(c["params"]))
    return arr, sp


def fold(m, c, arr, sp, near=0.0):
    """One search from a fresh record under the case's options: the record (amp, snr, id) as the device holds it."""
    with options(m.ctx, c):
        m.ctx.reset_best()
        if near > 0.0:
            with _near_window(m.ctx, near):
                m.ctx.match(arr, sp)
        else:
            m.ctx.match(arr, sp)
    return [a.copy() for a in m.ctx.get_best()]


def sub_result(best, win, c):
    """(amp, age, angle, snr) over a window, from the record: ids decoded as Matcher.result does, no template: zeros."""
    i0, i1, j0, j1 = win
    amp, snr, idx = (a[i0:i1, j0:j1] for a in best)
    p_of, a_of = dc.ids(c)
    none = idx >= len(p_of)
    k = np.where(none, 0, idx).astype(np.int64)
    assert not (none & ((amp != 0) | (snr != 0))).any()
    return amp.astype(float), np.where(none, 0.0, p_of[k]), np.where(none, 0.0, a_of[k]), snr.astype(float)


def check_case(best, c, stacks, what="fold"):
    chks = []
    for (label, win, _, a_st, s_st) in stacks:
        chk = dc.check_window(sub_result(best, win, c), c, a_st, s_st)
        assert chk["n_bad"] == 0, (c["name"], label, win, chk["n_bad"], np.argwhere(~chk["ok"])[:5])
        assert chk["n_inexact"] == 0, (c["name"], label, win, chk["n_inexact"])
        chks.append(chk)
        if chk["snr_err"] > 0.25 * chk["tie_rtol"]:             # (the windows that come near the policy's half window, by name)
            print("     %s, %s %s: snr_err=%.2e amp_err=%.2e, largest oracle SNR in the window %.3g"
                  % (c["name"], label, win, chk["snr_err"], chk["amp_err"], float(np.max(s_st))))
    report("%s%s" % (c["name"], "" if what == "fold" else " " + what), dc.merge_checks(chks), "direct")


def check_maps(amp, snr, c, stacks, t):
    """One template's maps over the case's windows: PARITY's value tolerances, as tests/test_gpu_tile_classes.py."""
    rtol, afac = orc.snr_tolerance(dc.FAMILIES[c["family"]][1])
    worst = [0.0, 0.0]
    for (label, (i0, i1, j0, j1), _, a_st, s_st) in stacks:
        o_amp, o_snr = a_st[t], s_st[t]
        d_a, d_s = np.abs(amp[i0:i1, j0:j1] - o_amp), np.abs(snr[i0:i1, j0:j1] - o_snr)
        ea = d_a - (P_AMP[0] * np.abs(o_amp) + P_AMP[1] * np.max(np.abs(a_st)))
        es = d_s - (rtol * np.abs(o_snr) + afac * np.max(s_st))
        assert (ea <= 1e-30).all() and (es <= 1e-30).all(), (c["name"], label, t, float(ea.max()), float(es.max()))
        assert (snr[i0:i1, j0:j1][o_snr == 0] == 0).all(), (c["name"], label, t)        # (masked cells: exactly zero)
        worst = [max(worst[0], float(d_a.max())), max(worst[1], float(d_s.max()))]
    print("maps %-44s template %d: max |d amp| %.2e, max |d snr| %.2e over %d windows" % (c["name"], t, worst[0], worst[1], len(stacks)))


@pytest.mark.parametrize("name", [c["name"] for c in dc.CASES])
def test_class_against_oracle(gpu_ctx, oracle_pool, name):
    """(a) the fold and one template's maps of a case, every cell of its windows (the small DEMs: of the grid)."""
    c = dc.CASE[name]
    stacks = dc.oracle_windows(c, oracle_pool)
    m = matcher(gpu_ctx, c["dem"])
    arr, sp = described(m, c)
    best = fold(m, c, arr, sp)
    check_case(best, c, stacks)
    # the public search is this search: Matcher.search(method="direct", exact=False) leaves the same record
    with options(gpu_ctx, c):
        m.search(dc.FAMILIES[c["family"]][0], c["scale"], c["params"], c["angles"], method="direct", exact=False)
        assert m.method_used == "direct"
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(best, gpu_ctx.get_best())), name
        # maps of one template: the last parameter (the largest window) at an oblique angle
        k = 1 * len(c["params"]) + len(c["params"]) - 1
        amp, snr = gpu_ctx.match_template(arr[k], sp)
    check_maps(amp, snr, c, stacks, int(arr[k].id))


# ---- (b) uploaded windows ------------------------------------------------------------------------------------------
def plugin(make):
    """A template class whose window the host uploads (no device descriptor): ``make()`` centred on the grid, no window
    limits - every cell of the DEM is live, the corners included."""
    class Uploaded(WT.Scarp):
        def _device_descriptor(self):
            return None

        def template(self):
            win = make()
            W = np.zeros((self.ny, self.nx))
            i0, j0 = self.ny // 2 - win.shape[0] // 2, self.nx // 2 - win.shape[1] // 2
            W[i0:i0 + win.shape[0], j0:j0 + win.shape[1]] = win
            return W

        def get_window_limits(self):
            return np.zeros((self.ny, self.nx), dtype=bool)
    return Uploaded


_WINDOW_ORACLE = {}
ANGLE_W = 0.4


def window_oracle(c):
    """orc.match_arrays of the case's window on its whole DEM, once per (DEM, window)."""
    W = c["make"]()
    key = (c["dem"], W.shape, float(np.sum(W)))
    if key not in _WINDOW_ORACLE:
        g = dc.dem(c["dem"])
        z = np.asarray(g._griddata, dtype=float)
        t = plugin(c["make"])(10, 1.0, ANGLE_W, z.shape[1], z.shape[0], 1.0)
        curv = orc.directional_curvature(z, 1.0, 1.0, ANGLE_W)
        o_amp, o_snr = orc.match_arrays(curv, t.template(), t.get_window_limits(), workers=8)
        o_amp.setflags(write=False)
        o_snr.setflags(write=False)
        _WINDOW_ORACLE[key] = (o_amp, o_snr)
    return _WINDOW_ORACLE[key]


def run_window(gpu_ctx, c, near=0.0):
    """The fold and the maps of a window case: (record, amp map, snr map)."""
    m = matcher(gpu_ctx, c["dem"])
    try:
        arr, bbox, max_area = m.describe(plugin(c["make"]), 10, np.array([1.0]), np.array([ANGLE_W]))
        assert (bbox[1] - bbox[0] + 1, bbox[3] - bbox[2] + 1) == dc.cropped_shape(c["make"]()), (c["name"], bbox)
        _, sp = m.plan_for(bbox, max_area, "direct", None)
        best = fold(m, c, arr, sp, near)
        with options(gpu_ctx, c):
            amp, snr = gpu_ctx.match_template(arr[0], sp)
        return best, amp, snr
    finally:
        gpu_ctx.clear_windows()


@pytest.mark.parametrize("name", [c["name"] for c in dc.WINDOW_CASES if c["dem"] != "L"])
def test_uploaded_window_against_oracle(gpu_ctx, name):
    """(b) the run-length window and the tall windows, fold and maps against orc.match_arrays on every cell of the DEM."""
    c = dc.WINDOW_CASE[name]
    o_amp, o_snr = window_oracle(c)
    best, amp, snr = run_window(gpu_ctx, c)
    one = dict(c, family="scarp", params=(1.0,), angles=(ANGLE_W,))
    ny, nx = o_amp.shape
    check_case(best, one, [("whole DEM", (0, ny, 0, nx), True, o_amp[None], o_snr[None])])
    # the maps are the record of a one-template search: the same bits
    assert np.array_equal(amp.view(np.uint32)[best[2] == 0], best[0].view(np.uint32)[best[2] == 0])
    assert np.array_equal(snr.view(np.uint32)[best[2] == 0], best[1].view(np.uint32)[best[2] == 0])
    check_maps(amp, snr, one, [("whole DEM", (0, ny, 0, nx), True, o_amp[None], o_snr[None])], 0)


# ---- (c) class independence ------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype.itemsize == 4 else a, b.view(np.uint32) if b.dtype.itemsize == 4 else b)


def differing(a, b):
    d = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    return len(d), d[:5].tolist()


@pytest.mark.parametrize("pair", dc.PAIRS, ids=["%s == %s" % p for p in dc.PAIRS])
def test_classes_agree_bit_for_bit(gpu_ctx, pair):
    """(c) one search through two classes (or slab counts, or batch regimes): the same record and maps in every bit."""
    ca, cb = dc.CASE[pair[0]], dc.CASE[pair[1]]
    assert all(ca[k] == cb[k] for k in ("dem", "family", "scale", "params", "angles"))
    assert (ca["classes"], ca["batched"], ca["variant"], ca["batch_off"]) != (cb["classes"], cb["batched"], cb["variant"], cb["batch_off"])
    m = matcher(gpu_ctx, ca["dem"])
    arr, sp = described(m, ca)
    recs = [fold(m, c, arr, sp) for c in (ca, cb)]
    for name, a, b in zip(("amp", "snr", "id"), *recs):
        assert same_bits(a, b), (pair, name) + differing(a, b)
    assert (recs[0][2] < len(arr)).any() and len(np.unique(recs[0][2])) > 2
    k = len(arr) - 1
    maps = []
    for c in (ca, cb):
        with options(gpu_ctx, c):
            maps.append(gpu_ctx.match_template(arr[k], sp))
    for name, a, b in zip(("map amp", "map snr"), *maps):
        assert same_bits(a, b), (pair, name) + differing(a, b)
    print("bits %-100s: record and maps identical (%d cells, %d templates)" % ("%s == %s" % pair, recs[0][0].size, len(arr)))


NEAR_PAIRS = [dc.PAIRS[0], dc.PAIRS[2], dc.PAIRS[5], dc.PAIRS[7]]


@pytest.mark.parametrize("pair", NEAR_PAIRS, ids=["%s == %s" % p for p in NEAR_PAIRS])
def test_near_window_leaves_the_record_and_flags_alike(gpu_ctx, pair):
    """(c) option "near_window" on (the exact mode's flags): the record is the same bits as with it off, and the flagged
    cells are the same in both classes."""
    ca, cb = dc.CASE[pair[0]], dc.CASE[pair[1]]
    m = matcher(gpu_ctx, ca["dem"])
    arr, sp = described(m, ca)
    plain = fold(m, ca, arr, sp)
    flags = []
    for c in (ca, cb):
        rec = fold(m, c, arr, sp, near=m.EXACT_WINDOW_DIRECT)
        for name, a, b in zip(("amp", "snr", "id"), plain, rec):
            assert same_bits(a, b), (pair, c["name"], name) + differing(a, b)
        flags.append(gpu_ctx.near_ties().copy())
    assert np.array_equal(flags[0], flags[1]), (pair, int((flags[0] != flags[1]).sum()))
    assert flags[0].any()
    print("near %-100s: record as without the flags, %d cells flagged in both" % ("%s == %s" % pair, int((flags[0] != 0).sum())))


@pytest.mark.parametrize("pair", dc.WINDOW_PAIRS, ids=["%s == %s" % p for p in dc.WINDOW_PAIRS])
def test_uploaded_window_classes_agree_bit_for_bit(gpu_ctx, pair):
    """(c) one uploaded window staged in one slab and in several (<1,2> against <2,2>), and in the W4 class against the
    whole LDS: the same record and maps in every bit."""
    ca, cb = dc.WINDOW_CASE[pair[0]], dc.WINDOW_CASE[pair[1]]
    assert ca["dem"] == cb["dem"] and np.array_equal(ca["make"](), cb["make"]())
    ra, rb = run_window(gpu_ctx, ca), run_window(gpu_ctx, cb)
    for name, a, b in zip(("amp", "snr", "id"), ra[0], rb[0]):
        assert same_bits(a, b), (pair, name) + differing(a, b)
    for name, a, b in zip(("map amp", "map snr"), ra[1:], rb[1:]):
        assert same_bits(a, b), (pair, name) + differing(a, b)
    assert (ra[0][1] > 0).any()
    print("bits %-100s: record and maps identical (%d cells)" % ("%s == %s" % pair, ra[0][0].size))
