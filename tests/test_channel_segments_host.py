"""sl.fit_channel_segments (docs/channels.md, "One width per reach") on the CPU: argument validation before the library is
loaded, the binding against its SIGNATURES entry through a recording fake library, the header's constants and struct sizes,
the kernels' budgets, the two numpy restatements (tests/channel_segment_reference.py) against each other on every input of
tests/test_gpu_channel_segments.py, the margins of the restatement's own decisions on them, and what the joint fit recovers
at a noise where the single-cell fit no longer does."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import channel_reference as cr
import channel_segment_reference as csr
from scarplet_amd import _lib
from test_fit_binding_host import fake_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 8.0, 6))
MARGIN = 1e-8                                                           # a decision closer than this is a near-tie


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_fit_channel_segments_validates_before_the_library_is_loaded(no_library, monkeypatch):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77, 90], labels=[1, 1, 2], angle=0.1, half_length=20.0, frequencies=FS)   # h = 10
    bad = [dict(depth="cell"), dict(depth=None), dict(depth=1), dict(max_shift=None), dict(max_shift=-1.0),
           dict(max_shift=20.0),                                          # D = 10 > h - min_samples
           dict(frequencies=[]), dict(frequencies=[0.1, 0.05]), dict(frequencies=[0.0, 0.1]), dict(frequencies=[np.nan]),
           dict(frequencies=np.linspace(0.01, 0.02, 65)), dict(frequencies=[6.1 / (2.0 * np.pi)]), dict(frequencies="f"),
           dict(labels=[1, 1]), dict(labels=[1.0, 1.0, 2.0]), dict(labels=[1, 1, 2 ** 31]), dict(labels=np.ones((3, 3), dtype=int)),
           dict(min_profiles=0), dict(min_profiles=1.5), dict(min_samples=0), dict(half_length=-1.0), dict(swath=-1.0),
           dict(cells=[3, 77, 40 * 50])]
    for kw in bad:
        with pytest.raises(ValueError):
            sl.fit_channel_segments(**dict(ok, **kw))
    # a reach above the park's cap: the cap is the header's formula, and the refusal comes before any upload
    from scarplet_amd import channel_segments
    h, F = 10, len(FS)
    assert _lib.channel_segment_park(h, F) == 8 * ((2 * h + 1) + 4 * F) + F
    assert _lib.channel_segment_cap(h, F) == _lib.SEGMENT_MAX_PARK // _lib.channel_segment_park(h, F)
    monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", 2 * _lib.channel_segment_park(h, F))
    with pytest.raises(ValueError, match="a segment of 3 cells: more than 2"):
        sl.fit_channel_segments(**dict(ok, labels=[4, 4, 4]))
    a = channel_segments.check_args((40, 50), 2.0, [3, 77, 90], [4, 4, 0], 0.1, 20.0, FS, 0, 4.0, "segment", 1.0, 4, 1)
    assert (a.D, a.mode, a.h) == (2, _lib.CHANNEL_DEPTH_SEGMENT, 10) and list(a.seg_start) == [0, 2] and list(a.kept) == [0, 1]
    # a matcher that holds a block is refused, as everywhere in the family
    from scarplet_amd import core

    class Block(object):
        whole = False
    with pytest.raises(ValueError, match="whole DEM"):
        core.Matcher.fit_channel_segments(Block(), None, 20.0, FS)


def test_the_tables_share_fit_channels_formulas():
    from scarplet_amd import channel_segments, channels
    assert channel_segments.FIT_DTYPE.names == ("label", "n_cells", "n_profiles", "n", "dof", "f_index", "lo_index", "hi_index",
                                                "status", "f", "f_lo", "f_hi", "a", "sse", "rmse", "depth", "sigma", "width",
                                                "width_lo", "width_hi", "area", "curvature")
    assert channel_segments.CELL_DTYPE.names == ("row", "col", "cell", "used", "n", "a", "b", "c0", "sse", "shift_index", "shift",
                                                 "depth", "centre_row", "centre_col", "label")
    # through a context that returns given rows: the derived fields are channels._table's, NaN where the row is not fitted
    rows = np.zeros(2, dtype=_lib.SEGMENT_FIT_DTYPE)
    rows["label"], rows["status"] = [1, 2], [0, 1]
    rows["kt"], rows["kt_lo"], rows["kt_hi"], rows["a"] = [0.05, np.nan], [0.04, np.nan], [0.07, np.nan], [-0.5, np.nan]

    class Ctx(object):
        def channel_segments(self, *a, **k):
            return rows, None, None, None
    args = channel_segments.check_args((40, 50), 1.0, [3, 77, 90], [1, 1, 2], 0.1, 10, [0.05], 0, 0, "profile", 1.0, 4, 1)
    t = channel_segments._run(Ctx(), args, 50, False, False, False)
    want = cr.derived(0.05, 0.04, 0.07, -0.5)
    for f in csr.DERIVED:
        assert t[f][0] == want[f], f
        assert np.isnan(t[f][1]), f
    assert t["f"][0] == 0.05 and t["f_lo"][0] == 0.04 and t["f_hi"][0] == 0.07 and list(t["label"]) == [1, 2]
    assert channels._table is not None


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_the_wrapper_fits_its_signature():
    K, F, S = 3, 2, 2
    cells, sa, ca = np.array([5, 7, 9], dtype=np.int64), np.array([0.0, 0.6, 0.8]), np.array([1.0, 0.8, 0.6])
    seg_start, seg_label = np.array([0, 2, 3], dtype=np.int64), np.array([1, 4], dtype=np.int32)
    freqs, z = np.array([0.05, 0.1]), np.arange(20.0).reshape(4, 5)
    ctx = fake_context()
    seen = set()
    for zz, tab, curve, plane in itertools.product((None, z), (False, True), (False, True), (False, True)):
        got = ctx.channel_segments(cells, sa, ca, seg_start, seg_label, freqs, 4, 1, 2, _lib.CHANNEL_DEPTH_SEGMENT, 1.5, 1.0, 2, 1,
                                   cell_table=tab, curve=curve, shift_plane=plane, z=zz)
        name, h, args = ctx.lib.log[-1]
        assert name == "sc_channel_segments" + ("_dem" if zz is not None else "")
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
        # K; S; F; h, w, D, mode, de, delta, min_samples, min_profiles
        assert own[3] == K and own[6] == S and own[8] == F and own[9:17] == (4, 1, 2, 1, 1.5, 1.0, 2, 1)
        rows, ct, sse, shifts = got
        assert rows.shape == (S,) and rows.dtype == _lib.SEGMENT_FIT_DTYPE
        assert (ct is None) == (not tab) and (sse is None) == (not curve) and (shifts is None) == (not plane)
        assert ct is None or (ct.shape == (K,) and ct.dtype == _lib.CHANNEL_SEGMENT_CELL_DTYPE)
        assert sse is None or (sse.shape == (S, F) and sse.dtype == np.float64 and sse.flags.c_contiguous)
        assert shifts is None or (shifts.shape == (K, F) and shifts.dtype == np.int8 and shifts.flags.c_contiguous)
    assert seen == {"sc_channel_segments", "sc_channel_segments_dem"}
    # the list is sc_fit_segments_shift's with the mode behind D ...
    for twin in ("", "_dem"):
        a, b = list(_lib.SIGNATURES["sc_channel_segments" + twin][1]), _lib.SIGNATURES["sc_fit_segments_shift" + twin][1]
        k = len(a) - 10
        assert a[k] is C.c_int and a[:k] + a[k + 1:] == b
    # ... and the names stay out of the fit family's count
    assert not [n for n in _lib.SIGNATURES if "channel" in n and n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_header_constants_and_abi(tmp_path):
    prog = tmp_path / "channel_segment.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n'
                    '  printf("%d %d %lld %lld %zu %zu %zu %d %d\\n", SC_CHANNEL_DEPTH_PROFILE, SC_CHANNEL_DEPTH_SEGMENT, '
                    '(long long)SC_CHANNEL_SEGMENT_PARK(100, 35), (long long)SC_SEGMENT_MAX_PARK, sizeof(sc_channel_segment_cell), '
                    'offsetof(sc_channel_segment_cell, shift_index), sizeof(sc_segment_fit), SC_K_COUNT, SC_ABI_VERSION);\n'
                    '  return 0;\n}\n')
    exe = tmp_path / "channel_segment"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    dt = _lib.CHANNEL_SEGMENT_CELL_DTYPE
    assert subprocess.check_output([str(exe)]).split() == [
        b"%d" % _lib.CHANNEL_DEPTH_PROFILE, b"%d" % _lib.CHANNEL_DEPTH_SEGMENT, b"%d" % _lib.channel_segment_park(100, 35),
        b"%d" % _lib.SEGMENT_MAX_PARK, b"%d" % dt.itemsize, b"%d" % dt.fields["shift_index"][1],
        b"%d" % _lib.SEGMENT_FIT_DTYPE.itemsize, b"%d" % len(_lib.K_NAMES), b"10"]
    # (the park stays under the bound of 8 ((2h + 1) + 6 F) + F bytes)
    assert dt.itemsize == 56 and _lib.channel_segment_park(100, 35) == 2763 <= 8 * (201 + 6 * 35) + 35
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in ("sc_channel_segments", "sc_channel_segments_dem"):
        assert re.search(r"\bint %s\s*\(" % n, code), n
    # the park's formula is stated once and the kernels' file refers to it
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_channel_segment.hip")).read()
    assert len(re.findall(r"#define\s+SC_CHANNEL_SEGMENT_PARK", txt)) == 1 and "SC_CHANNEL_SEGMENT_PARK" in src


def test_library_exports_the_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("sc_channel_segments", "sc_channel_segments_dem"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    a, b = _lib.SIGNATURES["sc_channel_segments"][1], _lib.SIGNATURES["sc_channel_segments_dem"][1]
    assert len(a) == 22 and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bsc_channel_segment\.hip\b", mk, flags=re.M)
    assert re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    assert "sc_channel.h" in re.search(r"^HDR\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    import scarplet_amd as sl
    assert callable(sl.fit_channel_segments) and callable(sl.Matcher.fit_channel_segments)


def test_kernel_budgets():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_channel_segment.hip")
    assert {"k_cs_stage<true>", "k_cs_stage<false>", "k_cs_choose"} <= set(t), sorted(t)
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
    for k in ("k_cs_stage<true>", "k_cs_stage<false>"):
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])              # four waves per SIMD
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_channel_segment.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src) and "atomic" not in re.sub(r"//.*", "", src)


# ---- the restatement against itself ----------------------------------------------------------------------------------------
def _both(case, mode):
    return csr.restate(case, mode), csr.restate(case, mode, longdouble=True)


@pytest.mark.parametrize("mode", csr.MODES)
def test_the_two_restatements_agree(mode):
    """One float64 lstsq on the full design matrix against the per-profile orthogonalised form in np.longdouble: the curves
    and the amplitude within RTOL / 100, no index decided differently, on every input the GPU tests use; the largest
    column-scaled condition number is below the family's."""
    worst, cond, fitted = 0.0, 0.0, 0
    for case in csr.gpu_cases() + [csr.recovery()]:
        for r, q in zip(*_both(case, mode)):
            for f in ("f_index", "lo_index", "hi_index", "status", "dof", "n", "n_profiles"):
                assert r[f] == q[f], (case["name"], r["label"], f, r[f], q[f])
            if r["status"] & 1:
                continue
            fitted += 1
            cv, cq = r["curve"], q["curve"]
            live = ~np.isnan(cv)
            assert np.array_equal(live, ~np.isnan(cq.astype(np.float64)))
            d = float(np.max(np.abs(cv[live] - cq[live]) / cq[live]))
            d = max(d, float(abs(r["a"] - q["a"]) / r["ptp"]))
            assert d <= csr.RTOL / 100, (case["name"], mode, r["label"], d)
            worst, cond = max(worst, d), max(cond, r["cond"])
    print("%s: %d fitted reaches, the restatements within %.2e, condition number at most %.1f" % (mode, fitted, worst, cond))
    assert fitted > 30 and cond < csr.COND_MAX


@pytest.mark.parametrize("mode", csr.MODES)
def test_no_case_lives_on_near_ties(mode):
    """The restatement's own margin of every decision - argmin, both walks, every d_ci - relative to the sse: no case has more
    than TIE_SHARE of its reaches with a margin below 1e-8."""
    for case in csr.gpu_cases() + [csr.recovery()]:
        rows = csr.restate(case, mode)
        near = [r["label"] for r in rows if r["margin"] < MARGIN]
        print("%-55s %-8s %2d reaches, smallest margin %.2e" % (case["name"], mode, len(rows), min([r["margin"] for r in rows],
                                                                                                  default=np.inf)))
        assert len(near) <= csr.TIE_SHARE * max(1, len(rows)), (case["name"], near)


def test_the_cases_cover_what_they_name():
    by = {c["name"]: c for c in csr.gpu_cases()}
    rows = csr.restate(by["sizes 1 2 63 64 65 129, h = 8, labels <= 0"], "profile")
    assert sorted(r["n_profiles"] for r in rows) == [1, 2, 63, 64, 65, 129] and all(r["status"] & 1 == 0 for r in rows)
    case = by["unusable cells, none usable, min_profiles 3, dof < 1"]
    for mode in csr.MODES:
        r = {x["label"]: x for x in csr.restate(case, mode)}
        assert list(r[3]["used"]) == [1, 1, 1, 1, 0, 0, 0, 1, 1, 1] and r[3]["status"] & 1 == 0
        assert r[1]["n_profiles"] == 0 and r[1]["status"] == 1
        assert r[8]["n_profiles"] == 2 and r[8]["dof"] >= 1 and r[8]["status"] == 1
        assert r[6]["n_profiles"] == 1 and r[6]["n"] == 4 and r[6]["dof"] < 1 and r[6]["status"] == 1
        assert r[4]["status"] & 1 == 0
    # complete and incomplete profiles in one reach
    case = by["NaN cells"]
    st = csr.stage_of(case)
    for _, pos in zip(*csr.group(case["labels"])):
        ns = {st[k]["n"] == 2 * case["h"] + 1 for k in pos if st[k]["usable"]}
        assert ns == {True, False}
    for mode in csr.MODES:
        a, b = csr.restate(by["a hole at the centre at pi f de = 6"], mode)
        assert list(np.flatnonzero(np.isnan(a["curve"]))) == [7] and not np.isnan(b["curve"]).any() and a["status"] & 1 == 0
        a, b = csr.restate(by["every frequency dead"], mode)
        assert a["status"] == (1 | 32) and b["status"] & 1 == 0
    assert len(by["F = 1"]["frequencies"]) == 1 and len(by["F = 64, h = 100, D = 8"]["frequencies"]) == 64
    c = by["F = 64, h = 100, D = 8"]
    assert 8 * (2 * (c["h"] + c["D"]) + 1) * 64 > 65536                   # the table leaves the LDS
    c = by["D = h - min_samples"]
    assert c["D"] == c["h"] - c["min_samples"]


def test_blocked_sum_is_the_stated_order():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((129, 3)) * 10.0 ** rng.integers(-8, 8, (129, 3))
    want = (np.add.accumulate(x[:64])[-1] + np.add.accumulate(x[64:128])[-1]) + x[128]
    assert np.array_equal(csr.blocked_sum(x), want)
    assert np.array_equal(csr.blocked_sum(x[:1]), x[0]) and np.isnan(csr.blocked_sum(np.array([[1.0], [np.nan], [2.0]]))).all()


# ---- what the joint fit recovers --------------------------------------------------------------------------------------------
def test_the_joint_fit_recovers_the_width_where_single_cells_do_not():
    """channel_reference.recovery_case's surface and its 100 offset cells as one reach, h = 100, w = 2, D = 8, at the first
    noise of the steps 0.3, 0.4, 0.5 at which the single-cell restatement finds the true index 14 in fewer than half the
    cells (docs/channels.md: 73, 64 and 49 of 100).  Both joint modes still return it."""
    case = csr.recovery()
    hits = csr.single_cell_hits(case)
    rows = {mode: csr.restate(case, mode)[0] for mode in csr.MODES}
    for mode, r in rows.items():
        print("noise %g, D = 8: single cells %d of 100; %s: index %d, interval [%d, %d], a %.5f, rmse %.5f, dof %d" %
              (csr.REC_NOISE, hits, mode, r["f_index"], r["lo_index"], r["hi_index"], r["a"], r["rmse"], r["dof"]))
    assert hits == csr.REC_HITS[-1] and hits < 50
    for r in rows.values():
        assert r["f_index"] == cr.REC["index"] == 14 and r["status"] & 1 == 0
    # without the shift, on the same cells: what the restatement shows - the off-centre cells widen the pooled trough by one
    # step of the grid and flatten it
    c0 = csr.recovery(D=0)
    h0 = csr.single_cell_hits(c0)
    for mode in csr.MODES:
        r = csr.restate(c0, mode)[0]
        print("noise %g, D = 0: single cells %d of 100; %s: index %d, interval [%d, %d], a %.5f" %
              (csr.REC_NOISE, h0, mode, r["f_index"], r["lo_index"], r["hi_index"], r["a"]))
        assert (r["f_index"], r["lo_index"], r["hi_index"]) == (13, 13, 13) and -0.88 < r["a"] < -0.87
    assert h0 == 22
