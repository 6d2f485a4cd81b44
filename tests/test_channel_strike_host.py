"""sl.fit_channels_along_strike (docs/channels.md, "Width along a reach") on the CPU: argument validation before the library
is loaded, the hand-over, the binding against its SIGNATURES entry through a recording fake library, the header, the Makefile
and the kernel's budget, the numpy restatement (tests/channel_strike_reference.py) on every input of
tests/test_gpu_channel_strike.py - no tie, both conditions on the inputs, what the cases cover - and the recovery: a trough
that doubles its width along the reach, whose stations return the planted width of their own cells."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import channel_reference as cr
import channel_strike_reference as cw
import strike_reference as stk
from scarplet_amd import _lib
from test_fit_binding_host import fake_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 8.0, 6))
SRC = "sc_channel_strike.hip"
CALLS = ("sc_channel_strike", "sc_channel_strike_dem")


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_arguments_validate_before_the_library_is_loaded(no_library, monkeypatch):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77, 90], labels=[1, 1, 2], angle=0.1, half_length=20.0, frequencies=FS, window=8.0)         # h = 10
    bad = [dict(depth="cell"), dict(depth=None), dict(max_shift=None), dict(max_shift=-1.0), dict(max_shift=20.0),
           dict(frequencies=[]), dict(frequencies=[0.1, 0.05]), dict(frequencies=[0.0, 0.1]), dict(frequencies=[np.nan]),
           dict(frequencies=np.linspace(0.01, 0.02, 65)), dict(frequencies=[6.1 / (2.0 * np.pi)]),
           dict(labels=[1, 1]), dict(labels=[1.0, 1.0, 2.0]), dict(min_profiles=0), dict(min_samples=0), dict(min_samples=11),
           dict(half_length=-1.0), dict(half_length=2.0), dict(swath=-1.0), dict(cells=[3, 77, 40 * 50]), dict(delta=-1.0),
           dict(angle=[0.1, np.nan, 0.1]), dict(data=np.zeros((40, 50))),
           dict(window=None), dict(window=1.9), dict(window=np.nan), dict(window=np.inf), dict(window="long"), dict(window=True),
           dict(step=1.9), dict(step=8.1), dict(step=np.nan), dict(step=np.inf), dict(step="short"), dict(window=3.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            sl.fit_channels_along_strike(**dict(ok, **kw))
            pytest.fail(str(kw))
    with pytest.raises(ValueError, match="window is required"):
        sl.fit_channels_along_strike(g, [3, 77], [1, 1], 0.1, 20.0, FS)     # window has no default
    # a reach above the park's cap is fit_channel_segments' refusal
    monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", 2 * _lib.channel_segment_park(10, len(FS)))
    with pytest.raises(ValueError, match="a segment of 3 cells: more than 2"):
        sl.fit_channels_along_strike(**dict(ok, labels=[4, 4, 4]))
    monkeypatch.undo()
    # what is valid gets as far as the device
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)
    for kw in (dict(), dict(step=2.0), dict(step=8.0), dict(window=2.0, step=2.0), dict(window=3.0, step=2.5), dict(max_shift=13.9),
               dict(depth="segment", return_curve=True, min_profiles=2, delta=0.0)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_channels_along_strike(**dict(ok, **kw))


def test_the_window_rules_are_stated_once():
    """fit_along_strike and fit_channels_along_strike take window and step through the same helper."""
    from scarplet_amd import channel_strike, strike
    assert strike.check_window(8.0, None, 2.0) == (8.0, 4.0) and strike.check_window(8, 2, 2.0) == (8.0, 2.0)
    for src in (strike.handover, channel_strike.check_args):
        names = src.__code__.co_names
        assert "check_window" in names and "cut" in names, src
    for mod in (strike, channel_strike):
        txt = open(mod.__file__).read()
        assert txt.count("window is required") == (1 if mod is strike else 0)


def test_the_hand_over_and_the_matcher_route():
    from scarplet_amd import channel_strike, core, strike, traces
    # cells 90 (row 1), 3 (row 0), 77 (row 1) of label 4 at orientation 0 lie at t = 2 row; 140 (row 2) too; label 0 is dropped
    a, where = channel_strike.check_args((40, 50), 2.0, [90, 3, 77, 5, 140], [4, 4, 4, 0, 4], 0.0, 20.0, FS, 0, 2.0, 2.0, 4.0,
                                         "segment", 2.0, 4, 1)
    assert (a.D, a.mode, a.h, a.delta) == (2, _lib.CHANNEL_DEPTH_SEGMENT, 10, 2.0)
    assert list(a.cells) == [3, 90, 77, 140] and list(a.seg_start) == [0, 4] and list(a.seg_label) == [4]
    # span 4, step 2 (the cell size): stations at t = 0, 2, 4, windows of |t - u| <= 1
    assert list(a.seg_win_start) == [0, 3] and list(a.win_lo) == [0, 1, 3] and list(a.win_hi) == [1, 3, 4]
    assert list(where[0]) == [0.0, 2.0, 4.0] and list(where[1]) == [0.0, 1.0, 2.0]
    assert a._fields[:8] == strike.Args._fields[:8] and a._fields[8] == "frequencies" and a._fields[12] == "mode"
    # the same cells through fit_along_strike's hand-over: the same order and the same windows
    b, where_b = strike.check_args((40, 50), 2.0, [90, 3, 77, 5, 140], [4, 4, 4, 0, 4], 0.0, 20.0, 0, 2.0, 2.0, [1.0], 2.0, 4, 1,
                                   4.0)
    for f in strike.Args._fields[:8]:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(window=1.0), dict(window=8.0, step=9.0), dict(window=8.0, step=1.0), dict(window=8.0, strike="both"),
               dict(window=8.0, min_profiles=0), dict(window=8.0, depth="reach"), dict(window=8.0, max_shift=None)):
        with pytest.raises(ValueError):
            core.Matcher.fit_channels_along_strike(Held(), tr, 20.0, FS, kw.pop("window"), strike=kw.pop("strike", "segment"), **kw)
    with pytest.raises(ValueError):
        core.Matcher.fit_channels_along_strike(Held(), "traces", 20.0, FS, 8.0)
    # a matcher that holds a block is refused, as everywhere in the family
    part = Held()
    part.whole = False
    with pytest.raises(ValueError, match="whole DEM"):
        core.Matcher.fit_channels_along_strike(part, tr, 20.0, FS, 8.0)


def test_the_table_fields():
    from scarplet_amd import channel_strike
    import scarplet_amd as sl
    assert channel_strike.FIT_DTYPE.names == (
        "label", "station", "n_cells", "n_profiles", "n", "dof", "f_index", "lo_index", "hi_index", "status", "f", "f_lo", "f_hi",
        "a", "sse", "rmse", "depth", "sigma", "width", "width_lo", "width_hi", "area", "curvature", "shift_mean", "t", "row", "col")
    assert sl.fit_channels_along_strike is channel_strike.fit_channels_along_strike
    assert callable(sl.Matcher.fit_channels_along_strike)
    rows = np.zeros(3, dtype=_lib.STRIKE_FIT_DTYPE)
    rows["label"], rows["station"], rows["status"], rows["n_profiles"] = 1, [0, 1, 2], [0, 1, 33], [4, 0, 2]
    for f, v in (("kt", 0.05), ("kt_lo", 0.04), ("kt_hi", 0.07), ("a", -0.5)):
        rows[f] = [v, np.nan, np.nan]

    class Ctx(object):
        def channel_strike(self, *a, **k):
            assert len(a) == 17 and k == dict(curve=False, z=None)
            return rows, None, np.array([-6, 0, 0], dtype=np.int32)
    args, where = channel_strike.check_args((40, 50), 2.0, [3, 53, 103], [1, 1, 1], 0.0, 20.0, [0.05], 0, 2.0, 2.0, 4.0, "profile",
                                            1.0, 4, 1)
    t = channel_strike._run(Ctx(), args, where, 50, False)
    want = cr.derived(0.05, 0.04, 0.07, -0.5)
    for f, v in want.items():
        assert t[f][0] == v and np.isnan(t[f][1]) and np.isnan(t[f][2]), f
    assert t["shift_mean"][0] == 2.0 * -6 / 4 and np.isnan(t["shift_mean"][1:]).all()
    assert list(t["t"]) == [0.0, 2.0, 4.0] and list(t["row"]) == [0.0, 1.0, 2.0] and list(t["col"]) == [3.0, 3.0, 3.0]


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_the_wrapper_fits_its_signature():
    K, F, S, NW = 3, 2, 2, 3
    cells, sa, ca = np.array([5, 7, 9], dtype=np.int64), np.array([0.0, 0.6, 0.8]), np.array([1.0, 0.8, 0.6])
    seg_start, seg_label = np.array([0, 2, 3], dtype=np.int64), np.array([1, 4], dtype=np.int32)
    sws, lo, hi = np.array([0, 2, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int64), np.array([1, 2, 3], dtype=np.int64)
    freqs, z = np.array([0.05, 0.1]), np.arange(20.0).reshape(4, 5)
    ctx = fake_context()
    seen = set()
    for zz, curve in itertools.product((None, z), (False, True)):
        got = ctx.channel_strike(cells, sa, ca, seg_start, seg_label, sws, lo, hi, freqs, 4, 1, 2, _lib.CHANNEL_DEPTH_SEGMENT, 1.5,
                                 0.5, 2, 1, curve=curve, z=zz)
        name, h, args = ctx.lib.log[-1]
        assert name == "sc_channel_strike" + ("_dem" if zz is not None else "")
        seen.add(name)
        argtypes = _lib.SIGNATURES[name][1]
        assert isinstance(h, C.c_void_p) and argtypes[0] is C.c_void_p and len(args) + 1 == len(argtypes)
        for i, a in enumerate(args):
            argtypes[i + 1].from_param(a)
            if argtypes[i + 1] is C.c_double:
                assert isinstance(a, float), (name, i, a)
            elif argtypes[i + 1] in (C.c_int, C.c_longlong):
                assert isinstance(a, int) and not isinstance(a, bool), (name, i, a)
            else:
                assert a is None or isinstance(a, argtypes[i + 1]), (name, i, a)
        own = args[3:] if zz is not None else args
        # K; S; NW; F; h, w, D, mode, de, delta, min_samples, min_profiles
        assert own[3] == K and own[6] == S and own[10] == NW and own[12] == F
        assert own[13:21] == (4, 1, 2, 1, 1.5, 0.5, 2, 1)
        rows, sse, ssum = got
        assert rows.shape == (NW,) and rows.dtype == _lib.STRIKE_FIT_DTYPE and ssum.shape == (NW,) and ssum.dtype == np.int32
        assert (sse is None) == (not curve) and (sse is None or (sse.shape == (NW, F) and sse.dtype == np.float64))
    assert seen == set(CALLS)
    # the list is sc_fit_strike's with the mode behind D and the sums of the shifts at the end
    for twin in ("", "_dem"):
        a, b = list(_lib.SIGNATURES["sc_channel_strike" + twin][1]), list(_lib.SIGNATURES["sc_fit_strike" + twin][1])
        k = len(b) - 6
        assert a[k] is C.c_int and a[:k] + a[k + 1:-1] == b and a[-1] is C.c_void_p
    assert not [n for n in _lib.SIGNATURES if "channel" in n and n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))]


# ---- the C ABI, the Makefile and the kernel --------------------------------------------------------------------------------------
def test_header_compiles_and_keeps_the_abi(tmp_path):
    prog = tmp_path / "channel_strike.c"
    prog.write_text('#include <stdio.h>\n#include "scarplet_hip.h"\nint main(void) {\n'
                    '  int (*f)(sc_ctx*, const long long*, const double*, const double*, long long, const long long*, const int32_t*,\n'
                    '           long long, const long long*, const long long*, const long long*, long long, const double*, int, int,\n'
                    '           int, int, int, double, double, int, int, sc_strike_fit*, double*, int32_t*) = sc_channel_strike;\n'
                    '  printf("%d %d %zu %d\\n", SC_K_COUNT, SC_ABI_VERSION, sizeof(sc_strike_fit), f != 0);\n  return 0;\n}\n')
    obj = tmp_path / "channel_strike.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(obj)])
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert len(_lib.SIGNATURES[n][1]) == 25 + (3 if n.endswith("_dem") else 0)
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


def test_library_exports_the_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    a, b = _lib.SIGNATURES[CALLS[0]][1], _lib.SIGNATURES[CALLS[1]][1]
    assert b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bsc_channel_strike\.hip\b", mk, flags=re.M)
    assert re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    assert "sc_strike.h" in re.search(r"^HDR\s*=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_kernel_budget():
    from test_isa_budget import kernel_table
    t = kernel_table(SRC)
    assert set(t) == {"k_cw_fit"}, sorted(t)                               # one new kernel
    r = t["k_cw_fit"]
    assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128, r           # four waves per SIMD
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "scarplet_amd", "csrc", SRC)).read())
    assert "asm" not in src and "atomic" not in src and "__shared__" not in src
    # Spp is k_st_spp's, reached through sc_strike.hip's launcher, and stage one sc_channel_segment.hip's
    assert "sc_st_spp_launch(" in src and "sc_cs_stage_launch(" in src and src.count("__global__") == 1
    # the kernels it stands on are where they were, with their budget
    s = kernel_table("sc_strike.hip")
    for k in ("k_st_spp", "k_st_fit"):
        assert k in s and s[k]["scratch"] == 0 and s[k]["vgpr"] + s[k]["agpr"] <= 128, (k, s.get(k))


# ---- the restatement on the inputs of tests/test_gpu_channel_strike.py -------------------------------------------------------------
def test_the_case_list():
    cases = cw.gpu_cases()
    assert [c["name"] for c in cases] == cw.NAMES and len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        assert c["z"].shape in ((96, 128), (300, 300), (256, 256)) and len(c["cells"]) <= 300
        assert 0 <= c["D"] <= min(_lib.PROFILE_MAX_SHIFT, c["h"] - c["min_samples"])
    assert sum(c["z"].shape == (256, 256) for c in cases) == 1
    by = {c["name"]: c for c in cases}
    for count, (window, step) in stk.RUNS.items():
        c = by["run %d" % count]
        assert (c["window"], c["step"]) == (window, step) and len(c["cells"]) == 200 and len(set(c["cells"] // 300)) == 200
    big = by["F = 64, h = 100, D = 8"]
    assert 8 * (2 * (big["h"] + big["D"]) + 1) * len(big["frequencies"]) > 65536          # the table is in global memory
    assert by["D = h - min_samples"]["D"] == by["D = h - min_samples"]["h"] - by["D = h - min_samples"]["min_samples"]
    assert by["de = 2"]["de"] == 2.0 and len(by["F = 1"]["frequencies"]) == 1 and by["D = 0"]["D"] == 0
    sev = by["several reaches"]
    assert sorted(set(sev["labels"][sev["labels"] > 0])) == [2, 5, 9, 11] and (sev["labels"] <= 0).sum() >= 3
    assert np.any(np.diff(sev["labels"]) < 0) and (sev["labels"] == 11).sum() == 1


@pytest.mark.parametrize("mode", cw.MODES)
@pytest.mark.parametrize("name", cw.NAMES)
def test_the_restatement_needs_no_tie(name, mode):
    """The tie cap must never be needed by the reference alone: on every input of the device's tests no decision of the
    restatement lies within RTOL, and every fitted window meets the conditions the tolerances stand on."""
    case = cw.gpu_cases()[cw.NAMES.index(name)]
    rows = cw.restate(case, mode)
    fit = [r for r in rows if r["status"] & 1 == 0]
    margin = min((r["margin"] for r in rows), default=np.inf)
    cond = max((r["cond"] for r in fit), default=0.0)
    spp = max((r["spp"] / np.nanmin(r["curve"]) for r in fit), default=0.0)
    print("%s, %s: %d windows, %d fitted, margin %.3g, cond %.3g, SSpp / sse %.3g" % (name, mode, len(rows), len(fit), margin, cond, spp))
    assert margin > cw.RTOL and cond <= cw.COND_MAX
    assert mode == "profile" or spp <= cw.SPP_MAX
    prof = np.array([r["n_profiles"] for r in rows])
    ncell = np.array([r["n_cells"] for r in rows])
    status = np.array([r["status"] for r in rows])
    dof = np.array([r["dof"] for r in rows])
    assert [(r["label"], r["station"]) for r in rows] == sorted((r["label"], r["station"]) for r in rows)
    if name.startswith("run"):
        assert int(name.split()[1]) in prof.tolist() and (status & 1 == 0).all(), prof
        assert any(r["shift_sum"] != 0 for r in rows)
    if name.startswith("unusable"):
        assert ((ncell == 0) & (status == 1)).any()                        # an empty window
        assert ((ncell > 0) & (prof == 0)).any()                           # cells, none usable
        assert ((prof > 0) & (prof < ncell) & (status & 1 == 0)).any()     # some unusable in a run
        assert ((prof >= 1) & (dof < 1) & (status == 1)).any()             # dof < 1
        sparse = (prof > 0) & (prof < 3) & (dof >= 1)
        assert sparse.any() and ((status[sparse] == 1) == (case["min_profiles"] == 3)).all()
        assert sorted(set(r["label"] for r in rows)) == [3, 7, 9]
    if name == "F = 1":
        assert (status[status & 1 == 0] & 6 == 6).all() and len(fit) > 0
    if name == "D = 0":
        assert not any(r["shift_sum"] for r in rows) and not (status & 8).any()
    if name == "several reaches":
        assert sorted(set(r["label"] for r in rows)) == [2, 5, 9, 11]
        assert [(r["n_cells"], r["station"]) for r in rows if r["label"] == 11] == [(1, 0)]
    if name == "NaN holes":
        # both routes of stage one in one window: complete and incomplete profiles
        st = cw.stage_of(case)
        np_full = 2 * case["h"] + 1
        assert any({True, False} <= {st[k]["n"] == np_full for k in r["where"] if st[k]["usable"]} for r in fit)
    F = len(case["frequencies"])
    if name == "a hole at the centre at pi f de = 6":
        holed = [40 in (case["cells"][r["where"]] // 128) for r in rows]
        assert any(holed) and not all(holed) and len(fit) == len(rows)
        for r, hd in zip(rows, holed):
            assert list(np.flatnonzero(np.isnan(r["curve"]))) == ([F - 1] if hd else []), (r["station"], hd)
    if name == "every frequency dead":
        holed = [40 in (case["cells"][r["where"]] // 128) for r in rows]
        assert [r["status"] for r in rows] == [33 if hd else 6 for hd in holed] and 33 in status and 6 in status


# ---- the recovery ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cw.MODES)
def test_the_stations_recover_the_planted_widths(mode):
    """The widening trough of "Intervals per reach" - the pooled fit returns 13 with [13, 13] and the bootstrap [12, 14] - in
    windows of 60 every 30: eleven stations, each returning the rounded mean of the planted index of its own cells, every
    interval one frequency wide; on the trough of constant width every station returns 13."""
    case = cw.recovery(3)
    rows = cw.restate(case, mode)
    assert [r["n_profiles"] for r in rows] == cw.REC_PROFILES and [r["station"] for r in rows] == list(range(11))
    idx = [r["f_index"] for r in rows]
    assert idx == cw.REC_INDEX[3] == [16, 15, 15, 14, 14, 13, 12, 12, 11, 11, 10]
    planted = cw.planted_index(case, 3)
    means = [float(planted[r["where"]].mean()) for r in rows]
    print(mode, idx, [round(m, 2) for m in means], min(r["margin"] for r in rows), max(r["cond"] for r in rows))
    assert idx == [int(np.floor(m + 0.5)) for m in means]
    assert all(r["lo_index"] == r["hi_index"] == r["f_index"] and r["status"] == 0 for r in rows)
    assert all(r["margin"] > cw.RTOL and r["cond"] <= cw.COND_MAX for r in rows)
    assert mode == "profile" or all(r["spp"] <= cw.SPP_MAX * np.nanmin(r["curve"]) for r in rows)
    flat = cw.restate(cw.recovery(0), mode)
    assert [r["f_index"] for r in flat] == cw.REC_INDEX[0] == [13] * 11
    assert all(r["margin"] > cw.RTOL and r["cond"] <= cw.COND_MAX for r in flat)
