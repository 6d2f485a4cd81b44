"""sl.bootstrap_along_strike on the CPU: argument validation before the library is loaded, the blocks of a window against a
plain loop, the draws against uint64 arithmetic, the layout of sc_strike_boot and the header's ABI, the kernel's register
budget, and the numpy restatement (tests/strike_bootstrap_reference.py) against strike_reference (replicate 0) and
bootstrap_reference (one window over a whole segment) on the noisy case of docs/segments.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bootstrap_reference as br
import segment_reference as sr
import strike_bootstrap_reference as sbr
import strike_reference as stk
from scarplet_amd import _lib, _plan, bootstrap, strike_bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()
CALLS = ("sc_strike_bootstrap", "sc_strike_bootstrap_dem")


# ---- every argument error is a ValueError before the library is loaded ---------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_arguments_validate_before_the_library_is_loaded(no_library):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77], labels=[1, 1], angle=0.1, half_length=20.0, window=8.0, block_length=2.0)     # h = 10
    bad = [
        # fit_along_strike's
        (dict(window=None), "window missing"),
        (dict(window=1.9), "window below the cell size"),
        (dict(window=np.nan), "window NaN"),
        (dict(window="long"), "window not a number"),
        (dict(step=1.9), "step below the cell size"),
        (dict(step=8.1), "step above the window"),
        (dict(step=np.inf), "step inf"),
        (dict(window=3.0), "window / 2 below the cell size and no step"),
        (dict(min_profiles=0), "min_profiles < 1"),
        (dict(min_samples=1), "min_samples < 2"),
        (dict(min_samples=11), "min_samples > h"),
        (dict(max_shift=-1.0), "max_shift < 0"),
        (dict(max_shift=14.0), "7 cells, more than h - min_samples = 6"),
        (dict(half_length=2.0), "h < 2"),
        (dict(swath=-1.0), "swath < 0"),
        (dict(ages=[3.0, 2.0]), "ages not increasing"),
        (dict(ages=[]), "no age"),
        (dict(cells=[3, 2000]), "a cell outside the grid"),
        (dict(labels=[1, 1, 1]), "labels of another length"),
        (dict(labels=[1.0, 1.0]), "labels not integers"),
        (dict(angle=[0.1, np.nan]), "angle NaN"),
        (dict(data=np.zeros((40, 50))), "data not a DEMGrid"),
        # bootstrap_segments'
        (dict(block_length=None), "block_length missing"),
        (dict(block_length=1.9), "block_length below the cell size"),
        (dict(block_length=np.nan), "block_length NaN"),
        (dict(block_length="long"), "block_length not a number"),
        (dict(replicates=0), "replicates < 1"),
        (dict(replicates=4097), "replicates > 4096"),
        (dict(replicates=10.5), "replicates not an integer"),
        (dict(level=0.0), "level 0"),
        (dict(level=1.0), "level 1"),
        (dict(level=np.nan), "level NaN"),
        (dict(seed=-1), "seed < 0"),
        (dict(seed=2 ** 64), "seed > 2^64 - 1"),
        (dict(seed=1.5), "seed not an integer"),
        (dict(min_blocks=1), "min_blocks < 2"),
        (dict(min_blocks=2.5), "min_blocks not an integer"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.bootstrap_along_strike(**dict(ok, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError):
        sl.bootstrap_along_strike(g, [3, 77], [1, 1], 0.1, 20.0, window=8.0)      # block_length has no default
    with pytest.raises(ValueError):
        sl.bootstrap_along_strike(g, [3, 77], [1, 1], 0.1, 20.0, block_length=2.0)     # nor has window
    # what is valid gets as far as the device
    for kw in (dict(), dict(step=2.0), dict(replicates=1), dict(replicates=4096, seed=2 ** 64 - 1), dict(level=0.5, min_blocks=2),
               dict(max_shift=13.9), dict(return_hist=True, min_profiles=2)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.bootstrap_along_strike(**dict(ok, **kw))


def test_a_window_whose_block_terms_exceed_64_kib_is_refused(no_library):
    """nb A 16 <= 65536: 64 ages hold 64 blocks.  A column of 120 cells at de = 1 (t = row, rows 40..159), blocks of one
    cell, stations every 32 at 51.5, 83.5, ...: a window of 63 holds the 64 rows 52..115, one of 66 the 66 rows 51..116."""
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((200, 60)), 1.0)
    cells = np.arange(40, 160) * 60 + 30
    kw = dict(labels=np.ones(120, dtype=int), angle=0.0, half_length=10.0, ages=10 ** np.linspace(0, 1.6, 64), step=32.0,
              block_length=1.0)
    a, _ = strike_bootstrap.check_args((200, 60), 1.0, cells, kw["labels"], 0.0, 10.0, 0, 63.0, 32.0, 1.0, 100, 0.95, 0, kw["ages"],
                                       4, 1, 5, None)
    assert np.diff(a.win_blk_start).max() == 64
    with pytest.raises(ValueError, match="block terms"):
        sl.bootstrap_along_strike(g, cells, window=66.0, **kw)
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.bootstrap_along_strike(g, cells, window=63.0, **kw)


def test_matcher_route_validates():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(window=1.0), dict(step=9.0), dict(block_length=1.0), dict(strike="both"), dict(replicates=0),
               dict(min_blocks=1)):
        args = dict(window=8.0, block_length=4.0)
        args.update(kw)
        with pytest.raises(ValueError):
            sl.Matcher.bootstrap_along_strike(Held(), tr, 20.0, args.pop("window"), args.pop("block_length"),
                                              strike=args.pop("strike", "segment"), **args)
    with pytest.raises(ValueError):
        sl.Matcher.bootstrap_along_strike(Held(), "traces", 20.0, 8.0, 4.0, strike="segment")
    part = Held()
    part.whole = False
    with pytest.raises(ValueError):
        sl.Matcher.bootstrap_along_strike(part, tr, 20.0, 8.0, 4.0, strike="segment")


def test_check_args_is_in_the_wrapper_s_order():
    import inspect
    a, where = strike_bootstrap.check_args((60, 50), 2.0, np.arange(10, 30) * 50 + 7, np.full(20, 4), 0.0, 20.0, 0, 12.0, None,
                                           4.0, 100, 0.95, 3, None, 4, 1, 2, None)
    params = list(inspect.signature(_lib.Context.strike_bootstrap).parameters)
    assert list(a._fields) == params[1:1 + len(a._fields)] and params[1 + len(a._fields):] == ["hist", "z"]
    assert a.R == 100 and a.seed == 3 and a.min_blocks == 2 and a.level == 0.95 and a.D == 0 and len(where) == 3
    # by hand (tests/test_strike_host.py): t = 20, 22, ... 58, windows [0, 4), [1, 7), ...; blocks of 4 hold two cells
    assert a.win_lo.tolist() == [0, 1, 4, 7, 10, 13, 16] and a.win_hi.tolist() == [4, 7, 10, 13, 16, 19, 20]
    assert a.win_blk_start.tolist() == [0, 2, 5, 8, 11, 14, 17, 19]
    assert a.blk_hi.tolist() == [2, 4, 3, 5, 7, 6, 8, 10, 9, 11, 13, 12, 14, 16, 15, 17, 19, 18, 20]
    assert a.win_blk_start.dtype == np.int64 and a.blk_hi.dtype == np.int64


def test_table_fields():
    assert strike_bootstrap.BOOT_DTYPE.names == (
        "label", "station", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "kt_index0", "lo_index", "hi_index",
        "status", "kt0", "kt_lo", "kt_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi", "height0", "height_lo", "height_hi", "t", "row",
        "col")
    import scarplet_amd as sl
    assert sl.bootstrap_along_strike is strike_bootstrap.bootstrap_along_strike and hasattr(sl.Matcher, "bootstrap_along_strike")


# ---- the blocks of a window -------------------------------------------------------------------------------------------------
def test_blocks_against_a_plain_loop():
    rng = np.random.default_rng(3)
    for trial in range(200):
        K = int(rng.integers(1, 80))
        t = np.sort(rng.choice([0.5, 1.0, 3.7]) * rng.integers(0, 60, K).astype(np.float64) + rng.choice([0.0, 0.25]))
        NW = int(rng.integers(1, 12))
        lo = np.sort(rng.integers(0, K + 1, NW))
        hi = np.minimum(lo + rng.integers(0, 30, NW), K)
        bl = float(rng.choice([0.5, 1.0, 2.0, 3.3, 100.0]))
        wb, bh = strike_bootstrap.blocks_of(t, lo, hi, bl)
        assert wb.dtype == np.int64 and bh.dtype == np.int64 and wb[0] == 0 and wb[-1] == len(bh)
        for g in range(NW):
            want = [lo[g] + e for _, e in sbr.blocks(t[lo[g]:hi[g]], bl)]
            assert bh[wb[g]:wb[g + 1]].tolist() == want, (trial, g)
            # the blocks tile the window: each holds a cell and the last ends where the window does
            edges = [lo[g]] + want
            assert all(b > a for a, b in zip(edges, edges[1:])) and edges[-1] == (hi[g] if hi[g] > lo[g] else lo[g])
    wb, bh = strike_bootstrap.blocks_of(np.zeros(0), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 1.0)
    assert wb.tolist() == [0] and len(bh) == 0
    # a stretch without a cell is no block: t = 0, 1, 7, 8 in blocks of 2 are two blocks, not five
    wb, bh = strike_bootstrap.blocks_of(np.array([0.0, 1.0, 7.0, 8.0]), [0], [4], 2.0)
    assert wb.tolist() == [0, 3] and bh.tolist() == [2, 3, 4]
    # one window over a whole segment: bootstrap.blocks_of
    t = np.sort(np.random.default_rng(4).uniform(0, 50, 40))
    b = np.floor((t - t[0]) / 3.0).astype(np.int64)
    wb, bh = strike_bootstrap.blocks_of(t, [0], [40], 3.0)
    assert bh.tolist() == (np.flatnonzero(np.diff(b)) + 1).tolist() + [40]


# ---- the draws ---------------------------------------------------------------------------------------------------------------
def test_draw_against_uint64_arithmetic():
    rng = np.random.default_rng(5)
    for seed, label, station, nb in [(0, 1, 0, 5), (7, 4, 3, 70), (2 ** 64 - 1, 2 ** 31 - 1, 2 ** 31 - 2, 4096), (123456789, 11, 1, 1)]:
        d = sbr.draws(seed, label, station, 40, nb)
        assert d.shape == (40, nb) and d.min() >= 0 and d.max() < nb
        for r, k in zip(rng.integers(1, 41, 30), rng.integers(0, nb, 30)):
            assert strike_bootstrap.draw(seed, label, station, int(r), int(k), nb) == d[r - 1, k]
    # station 0 has bootstrap_segments' key, another station has not
    for seed, label, nb in [(0, 1, 5), (7, 4, 70), (2 ** 64 - 1, 9, 13)]:
        mine = [strike_bootstrap.draw(seed, label, 0, r, k, nb) for r in range(1, 6) for k in range(nb)]
        assert mine == [bootstrap.draw(seed, label, r, k, nb) for r in range(1, 6) for k in range(nb)]
        assert np.array_equal(sbr.draws(seed, label, 0, 5, nb), br.draws(seed, label, 5, nb))
        assert mine != [strike_bootstrap.draw(seed, label, 1, r, k, nb) for r in range(1, 6) for k in range(nb)] or nb == 1


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_strike_boot, _lib.STRIKE_BOOT_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_strike_boot));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_strike_boot, %s));\n' % f for f in names)
    prog = tmp_path / "boot.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d\\n", SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "boot"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [11, 10]
    assert ctypes.sizeof(S) == 112 and dt.itemsize == 112 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert names == list(strike_bootstrap.BOOT_DTYPE.names[:19])


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    fit = _lib.SIGNATURES["sc_fit_strike"][1]
    for n in CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert not n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))
        # sc_fit_strike's arguments less delta, rows and curves; then the blocks, the resampling, rows and histograms
        assert len(_lib.SIGNATURES[n][1]) == len(fit) - 3 + 9 + (3 if n.endswith("_dem") else 0)
    own = _lib.SIGNATURES["sc_strike_bootstrap"][1]
    assert own[:18] == fit[:18] and own[-3] is ctypes.c_uint64 and own[-4] is ctypes.c_double
    assert _lib.BOOT_MAX_REPLICATES == 4096 and _lib.STRIKE_BOOT_LDS_TERMS == 65536
    assert re.search(r"#define\s+SB_LDS_TERMS\s+65536\b", open(os.path.join(ROOT, "scarplet_amd", "csrc",
                                                                            "sc_strike_bootstrap.hip")).read())


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_strike_bootstrap.hip" in src


def test_the_kernel_fits_its_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_strike_bootstrap.hip")
    assert sorted(t) == ["k_sb_window"], sorted(t)
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)                        # four waves per SIMD


# ---- the restatement on the noisy case of docs/segments.md ----------------------------------------------------------------
def noisy(window, step, bl, R, mb=5):
    z, cells, theta = sr.noisy_case()
    return z, cells, theta, sbr.bootstrap_along_strike(z, 1.0, cells, np.ones(100, dtype=int), theta, 100, 2, AGES, window, step,
                                                       bl, R, 0.95, 5, 0, 15, 1, mb)


def test_replicate_0_is_the_window_s_joint_fit():
    """Replicate 0 takes every block once: in every window of the noisy case (window 60, step 30: eleven stations of 11 to
    20 profiles, blocks of 10 - three or four profiles -, min_blocks 3) its index is strike_reference's kt_index and its a that fit's, to
    1e-9.  No replicate of the case lies within NEAR of a tie."""
    z, cells, theta, rows = noisy(60.0, 30.0, 10.0, 200, mb=3)
    ref = stk.fit_along_strike(z, 1.0, cells, np.ones(100, dtype=int), theta, 100, 2, AGES, 60.0, 30.0, min_samples=15)
    assert len(rows) == len(ref) == 11
    for r, f in zip(rows, ref):
        assert (r["label"], r["station"], r["n_cells"], r["n_profiles"]) == (f["label"], f["station"], f["n_cells"], f["n_profiles"])
        assert r["t"] == f["t"] and np.array_equal(r["where"], f["where"])
        assert r["status"] != 1 and f["status"] != 1 and r["n_blocks"] >= 3 and not r["near"].any()
        assert r["kt_index0"] == f["kt_index"], (r["station"], r["kt_index0"], f["kt_index"])
        assert abs(r["a0"] - f["a"]) <= 1e-9 * abs(f["a"]), (r["station"], r["a0"], f["a"])
        assert r["lo_index"] <= r["hi_index"] and r["a_lo"] <= r["a_mean"] <= r["a_hi"] and r["n_failed"] == 0
        assert r["hist"].sum() == 200


def test_one_window_over_a_segment_is_bootstrap_segments():
    """A window longer than the segment at a step as long: one station, number 0, whose key is bootstrap_segments'; its
    blocks are the segment's.  The integers and the histogram are bootstrap_reference's, the floats agree to 1e-9 (the
    profiles of a block are added in another order: along the strike here, in input order there); no replicate of
    either lies within NEAR of a tie."""
    z, cells, theta, rows = noisy(400.0, 400.0, 15.0, 300)
    ref = br.bootstrap_segments(z, 1.0, cells, np.ones(100, dtype=int), theta, 100, 2, AGES, 15.0, 300, 0.95, 5, 0, 15, 1, 5)
    assert len(rows) == 1 and len(ref) == 1
    r, f = rows[0], ref[0]
    assert r["station"] == 0 and r["n_blocks"] >= 20 and not r["near"].any() and not f["near"].any()
    for k in ("label", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "kt_index0", "lo_index", "hi_index", "status"):
        assert r[k] == f[k], (k, r[k], f[k])
    assert np.array_equal(r["hist"], f["hist"]) and np.array_equal(r["index"], f["index"])
    for k in ("kt0", "kt_lo", "kt_hi"):
        assert r[k] == f[k], k
    for k in ("a0", "a_mean", "a_sd", "a_lo", "a_hi"):
        assert abs(r[k] - f[k]) <= 1e-9 * abs(f[k]), (k, r[k], f[k])


def test_the_recovery_case_of_the_docs():
    """docs/strike.md, "Intervals per station": a scarp whose offset tapers linearly from 2 to 0.4 along 200 rows under
    noise of 0.3, windows of 30 every 10, blocks of 3, R = 500.  Of 20 stations the 95 % interval of the height holds the
    planted offset at 18; fit_along_strike's point estimate alone (replicate 0) lies within 5 % of it at 9."""
    z, cells, planted = sbr.taper_case()
    T = sbr.TAPER
    rows = sbr.bootstrap_along_strike(z, 1.0, cells, np.ones(200, dtype=int), 0.0, T["h"], T["w"], AGES, T["window"], T["step"],
                                      T["block_length"], T["R"], T["level"], T["seed"], 0, 4, 1, T["min_blocks"])
    assert not any(r["near"].any() for r in rows)
    assert sbr.taper_counts(rows, planted) == (20, 18, 9)
