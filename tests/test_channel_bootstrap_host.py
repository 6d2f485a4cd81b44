"""sl.bootstrap_channel_segments (docs/channels.md, "Intervals per reach") on the CPU: argument validation before the library
is loaded, the binding against its SIGNATURES entry through a recording fake library, the header's struct against gcc, the
kernels' budgets, the numpy restatement (tests/channel_bootstrap_reference.py) in float64 against itself in np.longdouble on
every input of tests/test_gpu_channel_bootstrap.py, the near-ties it finds on them, what the cases cover, and the widening
trough: a reach whose width changes downstream, on which the pooled interval stays one frequency wide and the bootstrap's
opens."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import bootstrap_reference as br
import channel_bootstrap_reference as cb
import channel_reference as cr
from scarplet_amd import _lib
from test_fit_binding_host import fake_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 8.0, 6))
SRC = "sc_channel_bootstrap.hip"


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_bootstrap_channel_segments_validates_before_the_library_is_loaded(no_library, monkeypatch):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77, 90], labels=[1, 1, 2], angle=0.1, half_length=20.0, frequencies=FS, block_length=4.0)   # h = 10
    bad = [dict(depth="cell"), dict(depth=None), dict(max_shift=None), dict(max_shift=-1.0), dict(max_shift=20.0),
           dict(frequencies=[]), dict(frequencies=[0.1, 0.05]), dict(frequencies=[0.0, 0.1]), dict(frequencies=[np.nan]),
           dict(frequencies=np.linspace(0.01, 0.02, 65)), dict(frequencies=[6.1 / (2.0 * np.pi)]),
           dict(labels=[1, 1]), dict(labels=[1.0, 1.0, 2.0]), dict(min_profiles=0), dict(min_samples=0), dict(half_length=-1.0),
           dict(swath=-1.0), dict(cells=[3, 77, 40 * 50]),
           dict(block_length=None), dict(block_length=1.9), dict(block_length=np.nan), dict(block_length="x"),
           dict(replicates=0), dict(replicates=4097), dict(replicates=2.5), dict(level=0.0), dict(level=1.0), dict(level=np.nan),
           dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(min_blocks=1), dict(min_blocks=2.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            sl.bootstrap_channel_segments(**dict(ok, **kw))
    # a reach above the park's cap is fit_channel_segments' refusal
    h, F = 10, len(FS)
    monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", 2 * _lib.channel_segment_park(h, F))
    with pytest.raises(ValueError, match="a segment of 3 cells: more than 2"):
        sl.bootstrap_channel_segments(**dict(ok, labels=[4, 4, 4]))
    monkeypatch.undo()
    from scarplet_amd import channel_bootstrap
    # the hand-over: cells 90 (row 1), 3 (row 0) and 77 (row 1) of label 4 at orientation 0 lie at t = 2 row; blocks of 2
    a = channel_bootstrap.check_args((40, 50), 2.0, [90, 3, 77, 5], [4, 4, 4, 0], 0.0, 20.0, FS, 0, 4.0, "segment", 2.0, 10, 0.9,
                                     2 ** 64 - 1, 4, 1, 2)
    assert (a.D, a.mode, a.h, a.R, a.level, a.seed, a.min_blocks) == (2, _lib.CHANNEL_DEPTH_SEGMENT, 10, 10, 0.9, 2 ** 64 - 1, 2)
    assert list(a.cells) == [3, 90, 77] and list(a.seg_start) == [0, 3] and list(a.seg_blk_start) == [0, 2]
    assert list(a.blk_start) == [0, 1, 3] and a._fields[:7] == ("cells", "sa", "ca", "seg_start", "seg_label", "seg_blk_start",
                                                                "blk_start")
    # a matcher that holds a block is refused, as everywhere in the family
    from scarplet_amd import core

    class Block(object):
        whole = False
    with pytest.raises(ValueError, match="whole DEM"):
        core.Matcher.bootstrap_channel_segments(Block(), None, 20.0, FS, 4.0)


def test_the_table_adds_fit_channels_formulas():
    from scarplet_amd import channel_bootstrap
    assert channel_bootstrap.BOOT_DTYPE.names == (
        "label", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "f_index0", "lo_index", "hi_index", "status", "f0",
        "f_lo", "f_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi", "area0", "area_mean", "area_sd", "area_lo", "area_hi", "depth0",
        "depth_lo", "depth_hi", "sigma0", "width0", "width_lo", "width_hi", "curvature0")
    rows = np.zeros(2, dtype=_lib.CHANNEL_BOOT_DTYPE)
    rows["label"], rows["status"] = [1, 2], [0, 1]
    for f, v in (("f0", 0.05), ("f_lo", 0.04), ("f_hi", 0.07), ("a0", -0.5), ("a_lo", -0.6), ("a_hi", -0.4)):
        rows[f] = [v, np.nan]

    class Ctx(object):
        def channel_bootstrap(self, *a, **k):
            assert len(a) == 19 and k == dict(hist=False, replicates=False, z=None)
            return rows, None, None, None
    args = channel_bootstrap.check_args((40, 50), 1.0, [3, 77, 90], [1, 1, 2], 0.1, 10, [0.05], 0, 0, "profile", 2.0, 10, 0.95, 0, 4,
                                        1, 5)
    t = channel_bootstrap._run(Ctx(), args, False, False)
    want = cr.derived(0.05, 0.04, 0.07, -0.5)
    for f, w in (("depth0", "depth"), ("sigma0", "sigma"), ("width0", "width"), ("width_lo", "width_lo"), ("width_hi", "width_hi"),
                 ("curvature0", "curvature")):
        assert t[f][0] == want[w] and np.isnan(t[f][1]), f
    assert (t["depth_lo"][0], t["depth_hi"][0]) == (0.4, 0.6) and t["width_lo"][0] < t["width0"][0] < t["width_hi"][0]
    assert channel_bootstrap.area_of(-0.5, 0.05) == cb.area_of(-0.5, 0.05) == want["area"]


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_the_wrapper_fits_its_signature():
    K, F, S, R = 3, 2, 2, 4
    cells, sa, ca = np.array([5, 7, 9], dtype=np.int64), np.array([0.0, 0.6, 0.8]), np.array([1.0, 0.8, 0.6])
    seg_start, seg_label = np.array([0, 2, 3], dtype=np.int64), np.array([1, 4], dtype=np.int32)
    seg_blk, blk = np.array([0, 2, 3], dtype=np.int64), np.array([0, 1, 2, 3], dtype=np.int64)
    freqs, z = np.array([0.05, 0.1]), np.arange(20.0).reshape(4, 5)
    ctx = fake_context()
    seen = set()
    for zz, hist, reps in itertools.product((None, z), (False, True), (False, True)):
        got = ctx.channel_bootstrap(cells, sa, ca, seg_start, seg_label, seg_blk, blk, freqs, 4, 1, 2, _lib.CHANNEL_DEPTH_SEGMENT, 1.5,
                                    2, 1, 2, R, 0.9, 2 ** 63 + 5, hist=hist, replicates=reps, z=zz)
        name, h, args = ctx.lib.log[-1]
        assert name == "sc_channel_bootstrap" + ("_dem" if zz is not None else "")
        seen.add(name)
        argtypes = _lib.SIGNATURES[name][1]
        assert isinstance(h, C.c_void_p) and argtypes[0] is C.c_void_p and len(args) + 1 == len(argtypes)
        for i, a in enumerate(args):
            argtypes[i + 1].from_param(a)
            if argtypes[i + 1] is C.c_double:
                assert isinstance(a, float), (name, i, a)
            elif argtypes[i + 1] in (C.c_int, C.c_longlong, C.c_uint64):
                assert isinstance(a, int) and not isinstance(a, bool), (name, i, a)
            else:
                assert a is None or isinstance(a, argtypes[i + 1]), (name, i, a)
        own = args[3:] if zz is not None else args
        # K; S; NB; F; h, w, D, mode, de, min_samples, min_profiles, min_blocks, R, level, seed
        assert own[3] == K and own[6] == S and own[9] == 3 and own[11] == F
        assert own[12:23] == (4, 1, 2, 1, 1.5, 2, 1, 2, R, 0.9, 2 ** 63 + 5)
        rows, hg, idx, amp = got
        assert rows.shape == (S,) and rows.dtype == _lib.CHANNEL_BOOT_DTYPE
        assert (hg is None) == (not hist) and (idx is None) == (not reps) and (amp is None) == (not reps)
        assert hg is None or (hg.shape == (S, F) and hg.dtype == np.int32 and hg.flags.c_contiguous)
        assert idx is None or (idx.shape == (S, R + 1) and idx.dtype == np.int8 and amp.shape == (S, R + 1) and amp.dtype == np.float64)
    assert seen == {"sc_channel_bootstrap", "sc_channel_bootstrap_dem"}
    # the list is sc_bootstrap_segments' with the mode behind D
    for twin in ("", "_dem"):
        a, b = list(_lib.SIGNATURES["sc_channel_bootstrap" + twin][1]), _lib.SIGNATURES["sc_bootstrap_segments" + twin][1]
        k = len(a) - 12
        assert a[k] is C.c_int and a[:k] + a[k + 1:] == b
    assert not [n for n in _lib.SIGNATURES if "channel" in n and n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_header_struct_and_abi(tmp_path):
    dt = _lib.CHANNEL_BOOT_DTYPE
    prog = tmp_path / "channel_boot.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n'
                    '  printf("%zu %d %d %d", sizeof(sc_channel_boot), SC_K_COUNT, SC_ABI_VERSION, SC_BOOT_MAX_REPLICATES);\n' +
                    "".join('  printf(" %%zu", offsetof(sc_channel_boot, %s));\n' % f for f in dt.names) +
                    '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "channel_boot"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"%d" % dt.itemsize, b"%d" % len(_lib.K_NAMES), b"10",
                                                           b"%d" % _lib.BOOT_MAX_REPLICATES] + [b"%d" % dt.fields[f][1] for f in dt.names]
    assert dt.itemsize == 144 and dt.names[:10] == _lib.SEGMENT_BOOT_DTYPE.names[:6] + ("f_index0", "lo_index", "hi_index", "status")
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in ("sc_channel_bootstrap", "sc_channel_bootstrap_dem"):
        assert re.search(r"\bint %s\s*\(" % n, code), n


def test_library_exports_the_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("sc_channel_bootstrap", "sc_channel_bootstrap_dem"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    a, b = _lib.SIGNATURES["sc_channel_bootstrap"][1], _lib.SIGNATURES["sc_channel_bootstrap_dem"][1]
    assert len(a) == 28 and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bsc_channel_bootstrap\.hip\b", mk, flags=re.M)
    assert re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    assert "sc_bootstrap.h" in re.search(r"^HDR\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    import scarplet_amd as sl
    assert callable(sl.bootstrap_channel_segments) and callable(sl.Matcher.bootstrap_channel_segments)


def test_kernel_budgets():
    from test_isa_budget import kernel_table
    t = kernel_table(SRC)
    assert {"k_cb_terms", "k_cb_reps<true>", "k_cb_reps<false>", "k_cb_summary"} <= set(t), sorted(t)
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)                       # four waves per SIMD
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "scarplet_amd", "csrc", SRC)).read())
    assert "asm" not in src
    # the one atomic is the integer histogram's, in LDS
    assert re.findall(r"atomic\w*\([^;]*;", src) == ["atomicAdd(&hist[idx], 1);"] and "__shared__ int hist[64]" in src
    # the scarp bootstrap's kernels are where they were, and the shared pieces are stated once
    old = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_bootstrap.hip")).read()
    hdr = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_bootstrap.h")).read()
    for k in ("k_bs_terms", "k_bs_reps", "k_bs_summary"):
        assert re.search(r"__global__[^;{]*\b%s\(" % k, old) and k + "(" not in src.replace("sc_bs_terms_launch", "")
    assert "bs_mix(unsigned long long z) {" in hdr and "bs_mix(unsigned long long z) {" not in old + src


# ---- the draws ---------------------------------------------------------------------------------------------------------------
def test_the_draws_are_bootstrap_segments():
    from scarplet_amd import bootstrap
    d = br.draws(7, 4, 5, 70)
    assert all(int(d[r - 1, k]) == bootstrap.draw(7, 4, r, k, 70) for r in (1, 5) for k in (0, 1, 63, 64, 69))
    p = cb.picks_of(7, 4, 5, 70)
    assert p.shape == (6, 70) and list(p[0]) == list(range(70)) and np.array_equal(p[1:], d)


# ---- the restatement against itself ----------------------------------------------------------------------------------------
def _cases():
    return cb.gpu_cases() + [cb.widening_case(s) for s in cb.WIDE_SPANS]


@pytest.mark.parametrize("mode", cb.MODES)
def test_the_two_restatements_agree(mode):
    """The replicates' sums in float64 against np.longdouble, on every input the GPU tests use: no index decided differently,
    a and area within RTOL / 100."""
    worst, booted = 0.0, 0
    for case in _cases():
        fs = case["frequencies"]
        for r, q in zip(cb.restate(case, mode), cb.restate(case, mode, longdouble=True)):
            assert np.array_equal(r["index"], q["index"]), (case["name"], r["label"], np.flatnonzero(r["index"] != q["index"])[:5])
            for f in ("f_index0", "lo_index", "hi_index", "status", "n_failed", "n_blocks", "n_profiles"):
                assert r[f] == q[f], (case["name"], r["label"], f, r[f], q[f])
            ok = r["index"] >= 0
            if not ok.any():
                continue
            booted += 1
            qa = q["a"][ok]
            d = float(np.max(np.abs(r["a"][ok] - qa) / np.abs(qa)))
            ar, aq = cb.area_of(r["a"][ok], fs[r["index"][ok]]), cb.area_of(qa, fs[q["index"][ok]].astype(np.longdouble))
            d = max(d, float(np.max(np.abs(ar - aq) / np.abs(aq))))
            if not r["status"] & 1:
                for f in ("a_mean", "a_lo", "a_hi", "area_mean", "area_lo", "area_hi"):
                    d = max(d, float(abs(r[f] - q[f]) / abs(q[f])))
            assert d <= cb.RTOL / 100, (case["name"], mode, r["label"], d)
            worst = max(worst, d)
    print("%s: %d reaches with replicates, the restatements within %.2e" % (mode, booted, worst))
    assert booted >= 20


@pytest.mark.parametrize("mode", cb.MODES)
def test_no_case_lives_on_near_ties(mode):
    """A replicate is a near-tie when its two best keys - Q_i in segment mode, SSse_i in profile mode - lie within 1e-12
    relative.  The cases' seeds and noise were chosen so that the restatement finds none at replicate 0 and at most 0.1 % of a
    case's replicates overall."""
    for case in _cases():
        rows = cb.restate(case, mode)
        n = sum(len(r["near"]) for r in rows if r["picks"] is not None)
        near = sum(int(r["near"].sum()) for r in rows)
        print("%-28s %-8s %5d replicates, %d near-ties" % (case["name"], mode, n, near))
        assert not any(r["near"][0] for r in rows), case["name"]
        assert near <= 1e-3 * max(1, n), (case["name"], near, n)


def test_the_cases_cover_what_they_name():
    by = {c["name"]: c for c in cb.gpu_cases()}
    assert list(by) == cb.NAMES
    for c in by.values():
        assert max(c["z"].shape) <= 160 and c["h"] <= 20 and len(c["cells"]) <= 300
    for mode in cb.MODES:
        r = {x["label"]: x for x in cb.restate(by["nb 1 4 5 70"], mode)}
        assert [r[l]["n_blocks"] for l in (6, 2, 9, 4)] == [1, 4, 5, 70] and [r[l]["status"] & 1 for l in (6, 2, 9, 4)] == [1, 1, 0, 0]
        assert cb.restate(by["R 1"], mode)[1]["hist"].sum() == 1 and np.isnan(cb.restate(by["R 1"], mode)[1]["a_sd"])
        assert cb.restate(by["R 1000"], mode)[1]["hist"].sum() == 1000
        assert cb.restate(by["F 1"], mode)[1]["status"] == 6
        r = cb.restate(by["a block of 130"], mode)[0]
        assert r["mb"].max() > 130 and r["status"] & 1 == 0
        r = cb.restate(by["an empty block"], mode)[0]
        assert (r["mb"] == 0).any() and not r["terms"][r["mb"] == 0].any() and r["status"] & 1 == 0
        r = cb.restate(by["clipped by the edge"], mode)[0]
        assert r["n_profiles"] < r["n_cells"] and r["status"] & 1 == 0
        # the dead frequency: dead in the third block alone; replicate 0 does not count it, the replicates that miss the block do
        # - and choose it, the trough being one cell wide -, and no replicate fails
        r = cb.restate(by["a dead frequency"], mode)[0]
        F = len(by["a dead frequency"]["frequencies"])
        assert list(np.flatnonzero(np.isnan(r["terms"][:, F - 1, 0]))) == [2] and not np.isnan(r["terms"][:, :F - 1]).any()
        miss = ~(r["picks"] == 2).any(axis=1)
        assert r["n_live"][0] == F - 1 and 0 <= r["index"][0] < F - 1 and r["n_failed"] == 0 and (r["index"] >= 0).all()
        assert np.array_equal(r["n_live"], np.where(miss, F, F - 1)) and np.array_equal(r["index"] == F - 1, miss)
        assert 40 < miss.sum() < 100
        # no live frequency: reach 1 in no replicate, reach 2 in all, reach 3 in those that miss its third block
        a, b, c = cb.restate(by["no live frequency"], mode)
        assert a["status"] == (1 | 32) and a["n_failed"] == a["replicates"] and a["n_blocks"] >= 5 and a["n_profiles"] == 30
        assert b["status"] == 6 and b["n_failed"] == 0
        miss = ~(c["picks"] == 2).any(axis=1)
        assert c["index"][0] == -1 and c["status"] == 6 and np.array_equal(c["index"] == 0, miss) and c["n_failed"] == (~miss[1:]).sum()
    c = by["F 64"]
    assert len(c["frequencies"]) == 64 and 70 * 64 * 16 > 65536 >= 5 * 64 * 16
    assert by["R 4096, F 64"]["R"] == _lib.BOOT_MAX_REPLICATES and len(by["R 4096, F 64"]["frequencies"]) == _lib.CHANNEL_MAX_FREQS
    assert by["D 3"]["D"] == 3 and by["nb 1 4 5 70"]["D"] == 0


# ---- the widening trough -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cb.MODES)
def test_the_bootstrap_opens_where_the_reach_is_not_one_width(mode):
    """docs/channels.md, "Intervals per reach": 100 cells along 300 rows of a 600 x 600 trough whose sigma is 1.5 * 1.12^(14 +
    span c) cells, c running from -1 to 1 along the strike.  fit_channel_segments' interval is one frequency wide at span 0 and
    at span 3 (a factor of 2 from end to end); the bootstrap's equals it at span 0 and strictly contains it at span 3."""
    for span in cb.WIDE_SPANS:
        case = cb.widening_case(span)
        p, r = cb.pooled(case, mode)[0], cb.restate(case, mode)[0]
        nz = np.flatnonzero(r["hist"])
        hist = (int(nz[0]), [int(v) for v in r["hist"][nz[0]:nz[-1] + 1]])
        print("span %g, %s: fit_channel_segments %d [%d, %d]; bootstrap %d [%d, %d], %d blocks, replicates from index %d: %s" %
              (span, mode, p["f_index"], p["lo_index"], p["hi_index"], r["f_index0"], r["lo_index"], r["hi_index"], r["n_blocks"],
               hist[0], hist[1]))
        assert p["status"] & 1 == 0 and r["status"] & 1 == 0 and r["n_failed"] == 0 and r["n_blocks"] == 11
        assert p["lo_index"] == p["hi_index"] == p["f_index"] == r["f_index0"]
        if span == 0:
            assert (r["lo_index"], r["hi_index"]) == (p["lo_index"], p["hi_index"])
        else:
            assert r["lo_index"] < p["lo_index"] and p["hi_index"] < r["hi_index"]
        assert hist == cb.WIDE_HIST[(span, mode)]
