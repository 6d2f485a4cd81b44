"""sl.bootstrap_channels_along_strike (docs/channels.md, "Intervals per station") on the CPU: argument validation before the
library is loaded - the 64 KiB refusal and every refusal of the two parents -, the Matcher route, the hand-over, the table,
the layout of sc_channel_strike_boot and the header's ABI, the Makefile, the kernel's budget and its LDS bound, the draws, and
the numpy restatement (tests/channel_strike_bootstrap_reference.py): against channel_strike_reference (replicate 0), against
channel_bootstrap_reference (one window over a reach) and against its longdouble twin on every input of
tests/test_gpu_channel_strike_bootstrap.py - what the cases cover, no case living on near-ties - and the recovery table of
the docs."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import channel_bootstrap_reference as cb
import channel_reference as cr
import channel_strike_bootstrap_reference as cwr
import channel_strike_reference as cw
import strike_bootstrap_reference as sbr
from scarplet_amd import _lib, bootstrap, channel_bootstrap, channel_strike, channel_strike_bootstrap, strike_bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 8.0, 6))
SRC = "sc_channel_strike_bootstrap.hip"
CALLS = ("sc_channel_strike_bootstrap", "sc_channel_strike_bootstrap_dem")


# ---- every argument error is a ValueError before the library is loaded ---------------------------------------------------------
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
    ok = dict(data=g, cells=[3, 77, 90], labels=[1, 1, 2], angle=0.1, half_length=20.0, frequencies=FS, window=8.0,
              block_length=2.0)                                             # h = 10
    bad = [
        # fit_channels_along_strike's
        dict(depth="cell"), dict(depth=None), dict(max_shift=None), dict(max_shift=-1.0), dict(max_shift=20.0),
        dict(frequencies=[]), dict(frequencies=[0.1, 0.05]), dict(frequencies=[0.0, 0.1]), dict(frequencies=[np.nan]),
        dict(frequencies=np.linspace(0.01, 0.02, 65)), dict(frequencies=[6.1 / (2.0 * np.pi)]),
        dict(labels=[1, 1]), dict(labels=[1.0, 1.0, 2.0]), dict(min_profiles=0), dict(min_samples=0), dict(min_samples=11),
        dict(half_length=-1.0), dict(half_length=2.0), dict(swath=-1.0), dict(cells=[3, 77, 40 * 50]),
        dict(angle=[0.1, np.nan, 0.1]), dict(data=np.zeros((40, 50))),
        dict(window=None), dict(window=1.9), dict(window=np.nan), dict(window=np.inf), dict(window="long"), dict(window=True),
        dict(step=1.9), dict(step=8.1), dict(step=np.nan), dict(step=np.inf), dict(step="short"), dict(window=3.0),
        # bootstrap_channel_segments'
        dict(block_length=None), dict(block_length=1.9), dict(block_length=np.nan), dict(block_length="long"),
        dict(replicates=0), dict(replicates=4097), dict(replicates=10.5), dict(level=0.0), dict(level=1.0), dict(level=np.nan),
        dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(min_blocks=1), dict(min_blocks=2.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            sl.bootstrap_channels_along_strike(**dict(ok, **kw))
            pytest.fail(str(kw))
    with pytest.raises(ValueError, match="window is required"):
        sl.bootstrap_channels_along_strike(g, [3, 77], [1, 1], 0.1, 20.0, FS, block_length=2.0)        # window has no default
    with pytest.raises(ValueError, match="block_length is required"):
        sl.bootstrap_channels_along_strike(g, [3, 77], [1, 1], 0.1, 20.0, FS, window=8.0)              # nor has block_length
    # a reach above the park's cap is fit_channel_segments' refusal
    monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", 2 * _lib.channel_segment_park(10, len(FS)))
    with pytest.raises(ValueError, match="a segment of 3 cells: more than 2"):
        sl.bootstrap_channels_along_strike(**dict(ok, labels=[4, 4, 4]))
    monkeypatch.undo()
    # what is valid gets as far as the device
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)
    for kw in (dict(), dict(step=2.0), dict(replicates=1), dict(replicates=4096, seed=2 ** 64 - 1), dict(level=0.5, min_blocks=2),
               dict(max_shift=13.9), dict(depth="segment", return_hist=True, min_profiles=2)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.bootstrap_channels_along_strike(**dict(ok, **kw))


def test_a_window_whose_block_terms_exceed_64_kib_is_refused(no_library):
    """nb F 16 <= 65536: 64 frequencies hold 64 blocks.  A column of 120 cells at de = 1 (t = row, rows 40..159), blocks of one
    cell, stations every 32 at 51.5, 83.5, ...: a window of 63 holds the 64 rows 52..115, one of 66 the 66 rows 51..116."""
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((200, 60)), 1.0)
    cells = np.arange(40, 160) * 60 + 30
    f64 = cr.freqs_of_sigma(np.geomspace(0.5, 20.0, 64))
    kw = dict(labels=np.ones(120, dtype=int), angle=0.0, half_length=10.0, frequencies=f64, step=32.0, block_length=1.0)
    a, _ = channel_strike_bootstrap.check_args((200, 60), 1.0, cells, kw["labels"], 0.0, 10.0, f64, 0, 63.0, 32.0, 1.0, 0, "profile",
                                               100, 0.95, 0, 4, 1, 5)
    assert np.diff(a.win_blk_start).max() == 64
    with pytest.raises(ValueError, match="block terms"):
        sl.bootstrap_channels_along_strike(g, cells, window=66.0, **kw)
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.bootstrap_channels_along_strike(g, cells, window=63.0, **kw)
    assert _lib.CHANNEL_STRIKE_BOOT_LDS_TERMS == 65536
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", SRC)).read()
    assert re.search(r"#define\s+CWB_LDS_TERMS\s+65536\b", src) and "SC_ERR_UNSUPPORTED" in \
        open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_strike.h")).read()


def test_matcher_route_validates():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(window=1.0), dict(step=9.0), dict(step=1.0), dict(block_length=1.0), dict(strike="both"), dict(replicates=0),
               dict(min_blocks=1), dict(min_profiles=0), dict(depth="reach"), dict(max_shift=None), dict(level=1.0)):
        args = dict(window=8.0, block_length=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            sl.Matcher.bootstrap_channels_along_strike(Held(), tr, 20.0, FS, args.pop("window"), args.pop("block_length"),
                                                       strike=args.pop("strike", "segment"), **args)
    with pytest.raises(ValueError):
        sl.Matcher.bootstrap_channels_along_strike(Held(), "traces", 20.0, FS, 8.0, 4.0, strike="segment")
    # a matcher that holds a block is refused, as everywhere in the family
    part = Held()
    part.whole = False
    with pytest.raises(ValueError, match="whole DEM"):
        sl.Matcher.bootstrap_channels_along_strike(part, tr, 20.0, FS, 8.0, 4.0)
    sig = inspect.signature(sl.Matcher.bootstrap_channels_along_strike)
    assert list(sig.parameters)[1:7] == ["traces", "half_length", "frequencies", "window", "block_length", "step"]
    assert sig.parameters["strike"].default == "cell" and sig.parameters["depth"].default == "profile"


def test_check_args_is_in_the_wrapper_s_order_and_shares_the_hand_over():
    cells, labels = np.arange(10, 30) * 50 + 7, np.full(20, 4)
    a, where = channel_strike_bootstrap.check_args((60, 50), 2.0, cells, labels, 0.0, 20.0, FS, 0, 12.0, None, 4.0, 4.0, "segment",
                                                   100, 0.95, 3, 4, 1, 2)
    params = list(inspect.signature(_lib.Context.channel_strike_bootstrap).parameters)
    assert list(a._fields) == params[1:1 + len(a._fields)] and params[1 + len(a._fields):] == ["hist", "z"]
    assert (a.R, a.seed, a.min_blocks, a.level, a.D, a.mode) == (100, 3, 2, 0.95, 2, _lib.CHANNEL_DEPTH_SEGMENT) and len(where) == 3
    # by hand (tests/test_strike_bootstrap_host.py): t = 20, 22, ... 58, windows [0, 4), [1, 7), ...; blocks of 4 hold two cells
    assert a.win_lo.tolist() == [0, 1, 4, 7, 10, 13, 16] and a.win_hi.tolist() == [4, 7, 10, 13, 16, 19, 20]
    assert a.win_blk_start.tolist() == [0, 2, 5, 8, 11, 14, 17, 19]
    assert a.blk_hi.tolist() == [2, 4, 3, 5, 7, 6, 8, 10, 9, 11, 13, 12, 14, 16, 15, 17, 19, 18, 20]
    assert a.win_blk_start.dtype == np.int64 and a.blk_hi.dtype == np.int64
    # everything shared with fit_channels_along_strike is that call's, byte for byte
    b, where_b, t = channel_strike.check_args((60, 50), 2.0, cells, labels, 0.0, 20.0, FS, 0, 12.0, None, 4.0, "segment", 0.0, 4, 1,
                                              with_t=True)
    for f in ("cells", "sa", "ca", "seg_start", "seg_label", "seg_win_start", "win_lo", "win_hi", "frequencies"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert all(x.tobytes() == y.tobytes() for x, y in zip(where, where_b))
    wb, bh = strike_bootstrap.blocks_of(t, b.win_lo, b.win_hi, 4.0)
    assert np.array_equal(wb, a.win_blk_start) and np.array_equal(bh, a.blk_hi)
    # nothing is validated twice: the parents' helpers are called, not restated
    names = channel_strike_bootstrap.check_args.__code__.co_names
    assert {"check_args", "check_resampling", "blocks_of"} <= set(names)
    txt = open(channel_strike_bootstrap.__file__).read()
    assert "is required" not in txt and "searchsorted" not in txt and "floor(" not in txt.replace("``floor(", "")


def test_the_table_fields_and_formulas():
    import scarplet_amd as sl
    raw = ("label", "station", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "f_index0", "lo_index", "hi_index",
           "status", "f0", "f_lo", "f_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi", "area0", "area_mean", "area_sd", "area_lo",
           "area_hi")
    assert _lib.CHANNEL_STRIKE_BOOT_DTYPE.names == raw
    assert channel_strike_bootstrap.BOOT_DTYPE.names == raw + (
        "depth0", "depth_lo", "depth_hi", "sigma0", "width0", "width_lo", "width_hi", "curvature0", "t", "row", "col")
    assert [n for n in raw if n != "station"] == list(_lib.CHANNEL_BOOT_DTYPE.names)
    assert sl.bootstrap_channels_along_strike is channel_strike_bootstrap.bootstrap_channels_along_strike
    assert callable(sl.Matcher.bootstrap_channels_along_strike)
    rows = np.zeros(3, dtype=_lib.CHANNEL_STRIKE_BOOT_DTYPE)
    rows["label"], rows["station"], rows["status"] = 1, [0, 1, 2], [0, 1, 33]
    for f, v in (("f0", 0.05), ("f_lo", 0.04), ("f_hi", 0.07), ("a0", -0.5), ("a_lo", -0.6), ("a_hi", -0.4)):
        rows[f] = [v, np.nan, np.nan]

    class Ctx(object):
        def channel_strike_bootstrap(self, *a, **k):
            assert len(a) == 22 and k == dict(hist=True, z=None)
            return rows, np.zeros((3, 1), dtype=np.int32)
    args, where = channel_strike_bootstrap.check_args((40, 50), 2.0, [3, 53, 103], [1, 1, 1], 0.0, 20.0, [0.05], 0, 2.0, 2.0, 2.0, 4.0,
                                                      "profile", 10, 0.9, 0, 4, 1, 2)
    t, hist = channel_strike_bootstrap._run(Ctx(), args, where, True)
    want = cr.derived(0.05, 0.04, 0.07, -0.5)
    for f, w in (("depth0", "depth"), ("sigma0", "sigma"), ("width0", "width"), ("width_lo", "width_lo"), ("width_hi", "width_hi"),
                 ("curvature0", "curvature")):
        assert t[f][0] == want[w] and np.isnan(t[f][1]) and np.isnan(t[f][2]), f
    assert t["width_lo"][0] < t["width0"][0] < t["width_hi"][0]            # width_lo comes from f_hi
    assert t["depth_lo"][0] == 0.4 and t["depth_hi"][0] == 0.6 and np.isnan(t["depth_lo"][1:]).all()
    assert list(t["t"]) == [0.0, 2.0, 4.0] and list(t["row"]) == [0.0, 1.0, 2.0] and list(t["col"]) == [3.0, 3.0, 3.0]
    # the same formulas as bootstrap_channel_segments' table
    seg = np.zeros(3, dtype=_lib.CHANNEL_BOOT_DTYPE)
    for f in seg.dtype.names:
        seg[f] = rows[f]

    class Seg(object):
        def channel_bootstrap(self, *a, **k):
            return seg, None, None, None
    s = channel_bootstrap._run(Seg(), [None] * 19, False, False)
    for f in cb.DERIVED:
        assert np.array_equal(t[f], s[f], equal_nan=True), f


# ---- the C ABI, the Makefile and the kernel --------------------------------------------------------------------------------------
def test_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_channel_strike_boot, _lib.CHANNEL_STRIKE_BOOT_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_channel_strike_boot));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_channel_strike_boot, %s));\n' % f for f in names)
    prog = tmp_path / "boot.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d\\n", SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "boot"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [11, 10]
    assert ctypes.sizeof(S) == 152 and dt.itemsize == 152 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert names == list(channel_strike_bootstrap.BOOT_DTYPE.names[:24])


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    sb = _lib.SIGNATURES["sc_strike_bootstrap"][1]
    for n in CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        # sc_strike_bootstrap's arguments with the depth mode behind D
        assert len(_lib.SIGNATURES[n][1]) == len(sb) + 1 + (3 if n.endswith("_dem") else 0)
    own = list(_lib.SIGNATURES[CALLS[0]][1])
    k = own.index(ctypes.c_double) - 1                                     # the mode stands before de
    assert own[k] is ctypes.c_int and own[:k] + own[k + 1:] == list(sb)
    a, b = _lib.SIGNATURES[CALLS[0]][1], _lib.SIGNATURES[CALLS[1]][1]
    assert b[:1] + b[4:] == a
    assert not [n for n in _lib.SIGNATURES if "channel" in n and n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))]


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert SRC in src and "sc_strike_bootstrap.hip" in src
    assert re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    assert "sc_strike.h" in re.search(r"^HDR\s*=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_the_kernel_fits_its_budget():
    from test_isa_budget import kernel_table
    t = kernel_table(SRC)
    assert sorted(t) == ["k_cwb_window<false>", "k_cwb_window<true>"], sorted(t)      # one kernel, a form per depth mode
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)                        # four waves per SIMD
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "scarplet_amd", "csrc", SRC)).read())
    assert "asm" not in src and src.count("__global__") == 1
    assert re.findall(r"atomic\w*", src) == ["atomicAdd"] and "atomicAdd(&hist[k], 1)" in src       # the integer histogram alone
    # stage one is sc_channel_segment.hip's, the draws sc_bootstrap.h's, the checks and the chunk's windows sc_strike.h's
    for call in ("sc_cs_stage_launch(", "bs_sums_counted<OWN>(", "sc_sb_check(", "sc_sb_windows(", "sc_cs_check(", "sc_sg_chunks("):
        assert call in src, call
    assert "sc_st_spp_launch" not in src and "k_sg_resid" not in src
    # sc_strike_bootstrap.hip shares them and does not keep a copy
    sib = re.sub(r"//.*", "", open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_strike_bootstrap.hip")).read())
    for name in ("sb_check", "sb_mix", "sb_sort_len"):
        assert not re.search(r"\b(int|long)\s+%s\s*\(" % name, sib), name
    assert "sc_sb_check(" in sib and "sc_sb_windows(" in sib


def test_the_lds_bound(tmp_path):
    """cwb_lds_bytes and its mirror: the worst accepted case - 64 KiB of terms at F = 1 (4096 blocks), R = 4096, profile mode -
    is 148 KiB of dynamic LDS and, with the kernel's 288 static bytes, within gfx950's 160 KiB; the workload of the docs is
    23 KB."""
    f = _lib.channel_strike_boot_lds
    worst = max(f(_lib.CHANNEL_STRIKE_BOOT_LDS_TERMS // (16 * F), F, R, own) for F in range(1, 65) for R in (1, 1000, 4096)
                for own in (False, True))
    assert worst == f(4096, 1, 4096, True) == 65536 + 16384 + 2 * 8 * 4096 + 4096 == 148 * 1024
    assert worst + _lib.CHANNEL_STRIKE_BOOT_LDS_STATIC <= _lib.LDS_BYTES == 160 * 1024
    assert f(10, 35, 1000, True) == 5600 + 17 * 1024 + 40 == 23048 and f(10, 35, 1000, False) == 23008
    assert f(3, 8, 1, False) == 16 * 24 + 17 * 2 and f(3, 8, 3, True) == 16 * 24 + 17 * 4 + 12      # the sort's length: 2, 4
    # the bound is computed in one host function
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", SRC)).read()
    assert len(re.findall(r"\bsize_t\s+cwb_lds_bytes\s*\(", src)) == 1
    # the static bytes are the compiler's
    hipcc = "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        out = str(tmp_path / "cwb.s")
        csrc = os.path.join(ROOT, "scarplet_amd", "csrc")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        os.path.join(csrc, SRC), "-o", out], check=True, capture_output=True, cwd=csrc)
        static = {int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", open(out).read())}
        assert static == {_lib.CHANNEL_STRIKE_BOOT_LDS_STATIC}, static


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def test_the_draws_are_strike_bootstrap_s():
    assert channel_strike_bootstrap.draw is strike_bootstrap.draw
    rng = np.random.default_rng(5)
    for seed, label, station, nb in [(0, 1, 0, 5), (7, 4, 3, 70), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 31 - 2, 4096), (123456789, 11, 1, 1)]:
        d = sbr.draws(seed, label, station, 40, nb)
        for r, k in zip(rng.integers(1, 41, 30), rng.integers(0, nb, 30)):
            assert channel_strike_bootstrap.draw(seed, label, station, int(r), int(k), nb) == d[r - 1, k]
    # station 0 has bootstrap_channel_segments' key (bootstrap_segments'), another station has not
    for seed, label, nb in [(0, 1, 5), (7, 4, 70)]:
        mine = [channel_strike_bootstrap.draw(seed, label, 0, r, k, nb) for r in range(1, 6) for k in range(nb)]
        assert mine == [bootstrap.draw(seed, label, r, k, nb) for r in range(1, 6) for k in range(nb)]
        assert mine != [channel_strike_bootstrap.draw(seed, label, 1, r, k, nb) for r in range(1, 6) for k in range(nb)]
    # the restatement draws the same blocks: a window's picks are the generator's
    case = cwr.gpu_cases()[cwr.NAMES.index("nb 1 4 5 70")]
    row = [r for r in cwr.restate(case, "segment") if r["label"] == 9][0]
    assert row["n_blocks"] == 5 and row["station"] == 0
    want = [[strike_bootstrap.draw(case["seed"], 9, 0, r, k, 5) for k in range(5)] for r in range(1, 4)]
    assert sbr.draws(case["seed"], 9, 0, 3, 5).tolist() == want


# ---- the restatement's anchors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cwr.MODES)
@pytest.mark.parametrize("name", ["R 1", "an empty block", "several reaches", "D 3"])
def test_replicate_0_is_the_window_s_fit(name, mode):
    """Replicate 0 takes every block once: in every window that both bootstrap and fit, its index is
    channel_strike_reference's f_index and its a that fit's, to 1e-9 - one lstsq per window and frequency there, block terms
    here."""
    case = cwr.gpu_cases()[cwr.NAMES.index(name)]
    rows = cwr.restate(case, mode)
    fit = cw.restate(dict(case, name="per station, " + name, delta=1.0), mode)
    assert len(rows) == len(fit) >= 6
    both = 0
    for r, f in zip(rows, fit):
        assert (r["label"], r["station"], r["n_cells"], r["n_profiles"]) == (f["label"], f["station"], f["n_cells"], f["n_profiles"])
        assert r["t"] == f["t"] and np.array_equal(r["where"], f["where"])
        if r["status"] & 1 or f["status"] & 1:
            continue
        both += 1
        assert r["f_index0"] == f["f_index"], (r["label"], r["station"], r["f_index0"], f["f_index"])
        assert abs(r["a0"] - f["a"]) <= 1e-9 * abs(f["a"]), (r["label"], r["station"], r["a0"], f["a"])
    assert both >= 6


@pytest.mark.parametrize("mode", cwr.MODES)
@pytest.mark.parametrize("name", ["nb 1 4 5 70", "runs 63 64 65", "a dead frequency", "no live frequency"])
def test_one_window_over_a_reach_is_the_reach_s_bootstrap(name, mode):
    """A step longer than the reach: one station, number 0, whose key is bootstrap_channel_segments'; its blocks are the
    reach's.  The integers and the histogram are channel_bootstrap_reference's, the floats agree to 1e-9 (the profiles of a
    block are added in another order: along the strike here, in input order there)."""
    case = cwr.gpu_cases()[cwr.NAMES.index(name)]
    rows = cwr.restate(case, mode)
    ref = cb.restate(dict(case, name="one window, " + name), mode)
    assert len(rows) == len(ref)
    for r, f in zip(rows, ref):
        assert r["station"] == 0 and not r["near"].any() and not f["near"].any()
        for k in ("label", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "f_index0", "lo_index", "hi_index", "status"):
            assert r[k] == f[k], (k, r[k], f[k])
        assert np.array_equal(r["hist"], f["hist"]) and np.array_equal(r["index"], f["index"]) and np.array_equal(r["mb"], f["mb"])
        for k in ("f0", "f_lo", "f_hi"):
            assert r[k] == f[k] or (np.isnan(r[k]) and np.isnan(f[k])), k
        for k in cb.ROW_FLOATS[3:]:
            if np.isnan(f[k]):
                assert np.isnan(r[k]), k
            else:
                assert abs(r[k] - f[k]) <= 1e-9 * abs(f[k]), (k, r[k], f[k])


@pytest.mark.parametrize("mode", cwr.MODES)
@pytest.mark.parametrize("name", cwr.NAMES)
def test_no_case_lives_on_near_ties_and_the_twin_agrees(name, mode):
    """The conditions the device's comparison stands on, asserted on the restatement alone: replicates whose two best keys
    lie within 1e-12 are at most 0.1 % of the case, none of them replicate 0; and the float64 restatement agrees with its
    longdouble twin - the same integers, floats within 1e-11 - so its own rounding is far below the family's 1e-9."""
    case = cwr.gpu_cases()[cwr.NAMES.index(name)]
    rows, twin = cwr.restate(case, mode), cwr.restate(case, mode, longdouble=True)
    reps = sum(r["replicates"] + 1 for r in rows if r["status"] & 1 == 0)
    near = sum(int(r["near"].sum()) for r in rows)
    worst = 0.0
    assert near <= 1e-3 * max(1, reps) and not any(r["near"][0] for r in rows)
    assert any(r["status"] & 1 == 0 for r in rows)
    for r, t in zip(rows, twin):
        assert not t["near"][0]
        for k in cwr.ROW_INTS + ("n_failed", "f_index0", "lo_index", "hi_index", "status"):
            assert r[k] == t[k] or r["near"].any() or t["near"].any(), (k, r[k], t[k])
        if r["near"].any() or t["near"].any():
            continue
        assert np.array_equal(r["index"], t["index"]) and np.array_equal(r["hist"], t["hist"])
        for k in cwr.ROW_FLOATS[3:]:
            if np.isnan(float(t[k])):
                assert np.isnan(float(r[k])), k
                continue
            scale = abs(float(t[k]))
            if k.endswith("_sd") and scale <= 1e-12 * abs(float(t[k[:-2] + "mean"])):
                scale = abs(float(t[k[:-2] + "mean"]))                      # (every replicate has the same value)
            d = abs(float(r[k]) - float(t[k])) / scale if scale else abs(float(r[k]))
            worst = max(worst, d)
            assert d <= 1e-11, (r["label"], r["station"], k, r[k], t[k])
    # the one window whose standard deviations are rounding alone, which compare holds against their means
    assert cwr.sd_rounding(rows) == ([(3, 10, "a_sd"), (3, 10, "area_sd")] if name == "empty windows" else [])
    if name == "empty windows":
        assert [r["mb"].tolist() for r in rows if (r["label"], r["station"]) == (3, 10)] == [[2, 0, 0]]
    print("%s, %s: %d windows, %d replicates, %d near, float64 against longdouble %.2g" % (name, mode, len(rows), reps, near, worst))


# ---- the case list ----------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_it_names():
    cases = cwr.gpu_cases()
    assert [c["name"] for c in cases] == cwr.NAMES and len(set(cwr.NAMES)) == len(cases)
    by = {c["name"]: c for c in cases}
    for c in cases:
        assert c["z"].shape == (160, 160) and c["h"] == 20 and len(c["cells"]) <= 300 and c["de"] == 1.0
        assert 0 <= c["D"] <= min(_lib.PROFILE_MAX_SHIFT, c["h"] - c["min_samples"])

    def rows(name, mode="profile"):
        return cwr.restate(by[name], mode)

    def col(name, f, mode="profile"):
        return [r[f] for r in rows(name, mode)]
    # the blocks of a window: 1, 4, 5 and 70 (a second round of 64 draws), and the min_blocks boundary at 5
    assert col("nb 1 4 5 70", "n_blocks") == [4, 70, 1, 5] and by["nb 1 4 5 70"]["min_blocks"] == 5
    assert [r["status"] & 1 for r in rows("nb 1 4 5 70")] == [1, 0, 1, 0]
    # the usable profiles of a block: 63, 64, 65 and 130
    assert [int(r["mb"][0]) for r in rows("runs 63 64 65")] == [63, 64, 65] and [int(r["mb"][0]) for r in rows("run 130")] == [130]
    assert all(r["mb"][1] == 3 and r["n_blocks"] == 2 for r in rows("runs 63 64 65") + rows("run 130"))
    # R: the sort lengths 2, 1024 and 4096; the ranks at the ends; the levels
    assert [by[n]["R"] for n in ("R 1", "R 1000", "R 4096")] == [1, 1000, 4096]
    assert (by["level 0.5"]["level"], by["level 0.999"]["level"]) == (0.5, 0.999)
    import bootstrap_reference as br
    assert br.ranks(100, 0.999) == (0, 99) and br.ranks(1, 0.95) == (0, 0) and br.ranks(100, 0.5) == (25, 74)
    # F and D
    assert len(by["F 1"]["frequencies"]) == 1 and len(by["F 64"]["frequencies"]) == 64 and by["D 3"]["D"] == 3
    assert all(by[n]["D"] == 0 for n in cwr.NAMES if n != "D 3")
    # windows and blocks: an empty block inside a bootstrapped window; an empty window; cells and no usable profile
    assert any((r["mb"] == 0).any() and (r["mb"] > 0).any() and r["status"] & 1 == 0 for r in rows("an empty block"))
    ew = rows("empty windows")
    assert sum(r["n_cells"] == 0 for r in ew) >= 2 and any(r["n_cells"] > 0 and r["n_profiles"] == 0 for r in ew)
    assert all(r["status"] == 1 and r["n_blocks"] == 0 for r in ew if r["n_cells"] == 0)
    # dead frequencies: dead in some replicates only; no live frequency at all, status 33; replicate 0 dead and others not
    for mode in cwr.MODES:
        d = rows("a dead frequency", mode)[0]
        F = len(by["a dead frequency"]["frequencies"])
        assert set(d["n_live"].tolist()) == {F - 1, F} and d["n_live"][0] == F - 1 and d["n_failed"] == 0
        n = rows("no live frequency", mode)
        assert [r["status"] for r in n] == [33, 6, 6] and n[0]["n_failed"] == 200 and 0 < n[2]["n_failed"] < 200
        assert n[2]["index"][0] == -1 and n[2]["f_index0"] == -1 and np.isnan(n[2]["a0"])
    # several reaches: two of a single cell, labels out of order
    sev = by["several reaches"]
    assert sorted(set(sev["labels"].tolist())) == [2, 4, 9, 11, 12] and np.any(np.diff(sev["labels"]) < 0)
    assert (sev["labels"] == 11).sum() == 1 and (sev["labels"] == 12).sum() == 1
    assert [(r["n_cells"], r["station"]) for r in rows("several reaches") if r["label"] == 11] == [(1, 0)]
    assert max(col("several reaches", "station")) >= 6
    # the caps: R = 4096, F = 64, 64 blocks - the 64 KiB of terms, to the byte
    caps = by["caps"]
    assert caps["R"] == 4096 and len(caps["frequencies"]) == 64 and max(col("caps", "n_blocks")) == 64
    a, _ = channel_strike_bootstrap.check_args(caps["z"].shape, 1.0, caps["cells"], caps["labels"], caps["angle"], 20.0,
                                               caps["frequencies"], float(caps["w"]), caps["window"], caps["step"],
                                               caps["block_length"], 0.0, "profile", 4096, 0.95, 7, 4, 1, 5)
    assert int(np.diff(a.win_blk_start).max()) * 64 * 16 == _lib.CHANNEL_STRIKE_BOOT_LDS_TERMS
    # the host cuts the blocks the restatement cuts, in every case
    for c in cases:
        a, _ = channel_strike_bootstrap.check_args(c["z"].shape, c["de"], c["cells"], c["labels"], c["angle"], float(c["h"]),
                                                   c["frequencies"], float(c["w"]), c["window"], c["step"], c["block_length"],
                                                   float(c["D"]), "profile", c["R"], c["level"], c["seed"], c["min_samples"],
                                                   c["min_profiles"], c["min_blocks"])
        assert np.diff(a.win_blk_start).tolist() == col(c["name"], "n_blocks"), c["name"]
        assert (a.win_hi - a.win_lo).tolist() == col(c["name"], "n_cells"), c["name"]


# ---- the recovery table of the docs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cwr.MODES)
def test_the_recovery_table_of_the_docs(mode):
    """docs/channels.md, "Intervals per station": the widening trough of "Intervals per reach" in windows of 60 every 30 -
    the eleven stations of "Width along a reach", whose pooled intervals are one frequency wide - in blocks of 9 (three
    profiles; 4 to 7 blocks a window, min_blocks 3), R = 1000.  As the restatement returns them, in both depth modes: at
    span 3 eight of the eleven intervals are two frequencies wide, and every one holds the station's own f_index; at span 0
    nine are [13, 13] and two [13, 14]."""
    for span in (3, 0):
        rows = cwr.restate(cwr.recovery(span), mode)
        assert [r["n_profiles"] for r in rows] == cw.REC_PROFILES and [r["station"] for r in rows] == list(range(11))
        assert [r["n_blocks"] for r in rows] == [4] + [7] * 9 + [4] and all(r["status"] == 0 and r["n_failed"] == 0 for r in rows)
        assert [r["f_index0"] for r in rows] == cw.REC_INDEX[span]
        got = [[r["lo_index"], r["hi_index"]] for r in rows]
        print(span, mode, got, [round(float(r["a_mean"]), 4) for r in rows])
        assert got == cwr.REC_INTERVALS[span]
        assert all(lo <= i0 <= hi for (lo, hi), i0 in zip(got, cw.REC_INDEX[span]))
        assert not any(r["near"].any() for r in rows)
