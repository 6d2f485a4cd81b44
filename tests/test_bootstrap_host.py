"""sl.bootstrap_segments on the CPU: the draw against hand-computed values, the blocks along the strike, argument
validation before the library is loaded, the layout of sc_segment_boot and the header's ABI, the exported symbols, the
kernels' register budget, and the numpy restatement (tests/bootstrap_reference.py) on the noisy case of
docs/segments.md."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bootstrap_reference as br
import segment_reference as sr
from scarplet_amd import _lib, _plan, bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()


# ---- the draw ----------------------------------------------------------------------------------------------------------
# (seed, label, r, k, nb) -> block, worked out by hand with Python integers from the definition in docs/bootstrap.md; the
# keys mix(seed ^ label * 0x9E3779B97F4A7C15) of the three are 0xe220a8397b1dcdaf, 0x9378b9d8ea31f81d, 0x0ac268c4f9a57ed2
DRAWS = [((0, 1, 1, 0, 5), 0), ((12345, 7, 1000, 69, 70), 36), ((2 ** 64 - 1, 2 ** 31 - 1, 4096, 3, 1000), 503)]


def test_draw_against_hand_computed_values():
    assert bootstrap.mix(0 ^ (1 * 0x9E3779B97F4A7C15)) == 0xe220a8397b1dcdaf
    assert bootstrap.mix(12345 ^ (7 * 0x9E3779B97F4A7C15)) == 0x9378b9d8ea31f81d
    for (seed, label, r, k, nb), want in DRAWS:
        assert bootstrap.draw(seed, label, r, k, nb) == want
        assert br.draws(seed, label, r, nb)[r - 1, k] == want             # the restatement's uint64 arithmetic
    assert br.draws(0, 1, 1, 5).tolist() == [[0, 1, 3, 2, 4]]
    d = br.draws(3, 9, 200, 7)
    assert d.min() == 0 and d.max() == 6
    assert all(bootstrap.draw(3, 9, r, k, 7) == d[r - 1, k] for r in (1, 77, 200) for k in range(7))


# ---- the blocks ----------------------------------------------------------------------------------------------------------
def handover(shape, de, cells, labels, angle, block_length, **kw):
    a = bootstrap.check_args(shape, de, cells, labels, angle, 10.0 * de, 0, block_length, 10, 0.9, 0, AGES, 4, 1, 2, None, **kw)
    return dict(zip(("cells", "sa", "ca", "seg_start", "seg_label", "seg_blk_start", "blk_start"), a[:7]))


def test_blocks_on_a_vertical_line():
    """Strike 0: t = de row.  Twenty cells of one column at de = 2 in blocks of 6: three rows to a block."""
    nx = 50
    rows = np.arange(10, 30)
    perm = np.random.default_rng(1).permutation(20)
    cells = (rows * nx + 7)[perm]
    h = handover((60, nx), 2.0, cells, np.full(20, 4), 0.0, 6.0)
    assert h["seg_label"].tolist() == [4] and h["seg_start"].tolist() == [0, 20] and h["seg_blk_start"].tolist() == [0, 7]
    assert h["blk_start"].tolist() == [0, 3, 6, 9, 12, 15, 18, 20]
    got = h["cells"] // nx
    assert sorted(got.tolist()) == rows.tolist()
    for b in range(7):
        blk = got[h["blk_start"][b]:h["blk_start"][b + 1]]
        assert set(blk.tolist()) == set(range(10 + 3 * b, min(10 + 3 * b + 3, 30)))
        # input order is kept within a block
        assert blk.tolist() == [r for r in rows[perm].tolist() if r in set(blk.tolist())]
    ref = br.blocks(cells, nx, 2.0, br.strike_of(np.zeros(20)), 6.0)
    assert [cells[p].tolist() for p in ref] == [h["cells"][h["blk_start"][b]:h["blk_start"][b + 1]].tolist() for b in range(7)]


def test_blocks_on_a_diagonal():
    """Strike pi / 4, cells (r, r): t = r sqrt(2) de, blocks of 3."""
    nx = 40
    r = np.arange(5, 25)
    cells = r * nx + r
    h = handover((40, nx), 1.0, cells, np.ones(20, dtype=int), np.pi / 4, 3.0)
    want = [int(math.floor((v - 5) * math.sqrt(2.0) / 3.0)) for v in r]
    assert len(set(want)) == 9 and h["seg_blk_start"].tolist() == [0, 9]
    assert np.diff(h["blk_start"]).tolist() == [want.count(b) for b in range(9)]
    assert np.array_equal(h["cells"], cells)
    # two segments, interleaved, with a gap along the second: blocks that hold no cell are not blocks
    lab = np.where(np.arange(20) % 2 == 0, 2, 1)
    cells2 = cells.copy()
    cells2[lab == 1] = np.array([5, 6, 7, 30, 31, 32, 33, 34, 35, 36]) * nx + 3      # a vertical line with a hole of 22 rows
    ang = np.where(lab == 1, 0.0, np.pi / 4)
    h = handover((40, nx), 1.0, cells2, lab, ang, 3.0)
    assert h["seg_label"].tolist() == [1, 2] and h["seg_start"].tolist() == [0, 10, 20]
    assert h["seg_blk_start"].tolist() == [0, 4, 4 + len({want[i] for i in range(0, 20, 2)})]
    assert np.diff(h["blk_start"])[:4].tolist() == [3, 2, 3, 2]            # rows 5-7 | 30-31 | 32-34 | 35-36: blocks 0, 8, 9, 10
    assert h["blk_start"][-1] == 20
    for L, seg in ((1, 0), (2, 1)):
        ref = br.blocks(cells2[lab == L], nx, 1.0, br.strike_of(ang[lab == L]), 3.0)
        b0 = h["seg_blk_start"][seg]
        assert [cells2[lab == L][p].tolist() for p in ref] == \
            [h["cells"][h["blk_start"][b0 + b]:h["blk_start"][b0 + b + 1]].tolist() for b in range(len(ref))]


def test_segment_strike_is_the_axial_mean():
    a = np.array([0.1, 0.3, 0.2 + np.pi, 0.2 - np.pi])
    s = bootstrap.segment_strikes(a, np.array([0, 4]))
    assert abs(s[0] - 0.2) < 1e-12 and s[0] == br.strike_of(a)
    # a given strike per label takes its place (the Matcher's strike="segment")
    nx = 50
    cells = np.arange(10, 30) * nx + 7
    h = handover((60, nx), 1.0, cells, np.full(20, 2), 1.0, 5.0, seg_strike=np.array([9.9, 0.0]))
    assert np.diff(h["blk_start"]).tolist() == [5, 5, 5, 5]


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
    ok = dict(data=g, cells=[3, 77], labels=[1, 1], angle=0.1, half_length=20.0, block_length=4.0)    # h = 10
    bad = [
        (dict(block_length=None), "block_length missing"),
        (dict(block_length=1.9), "block_length below the cell size"),
        (dict(block_length=np.nan), "block_length NaN"),
        (dict(block_length=np.inf), "block_length inf"),
        (dict(block_length="long"), "block_length not a number"),
        (dict(block_length=True), "block_length a bool"),
        (dict(replicates=0), "no replicate"),
        (dict(replicates=4097), "too many replicates"),
        (dict(replicates=10.5), "replicates not an integer"),
        (dict(replicates=True), "replicates a bool"),
        (dict(level=0.0), "level 0"),
        (dict(level=1.0), "level 1"),
        (dict(level=np.nan), "level NaN"),
        (dict(level="high"), "level not a number"),
        (dict(seed=-1), "seed < 0"),
        (dict(seed=2 ** 64), "seed beyond 64 bits"),
        (dict(seed=1.5), "seed not an integer"),
        (dict(min_blocks=1), "min_blocks < 2"),
        (dict(min_blocks=2.5), "min_blocks not an integer"),
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
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.bootstrap_segments(**dict(ok, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError):
        sl.bootstrap_segments(g, [3, 77], [1, 1], 0.1, 20.0)               # block_length has no default
    # what is valid gets as far as the device
    for kw in (dict(), dict(replicates=1), dict(replicates=4096, level=0.5, seed=2 ** 64 - 1, min_blocks=2),
               dict(block_length=2.0, max_shift=13.9), dict(max_shift=0), dict(return_hist=True, return_replicates=True)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.bootstrap_segments(**dict(ok, **kw))


def test_matcher_route_validates():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(block_length=1.0), dict(block_length=4.0, replicates=0), dict(block_length=4.0, level=2.0),
               dict(block_length=4.0, strike="both"), dict(block_length=4.0, min_blocks=1)):
        with pytest.raises(ValueError):
            sl.Matcher.bootstrap_segments(Held(), tr, 20.0, strike=kw.pop("strike", "segment"), **kw)
    with pytest.raises(ValueError):
        sl.Matcher.bootstrap_segments(Held(), "traces", 20.0, 4.0)
    part = Held()
    part.whole = False
    with pytest.raises(ValueError):
        sl.Matcher.bootstrap_segments(part, tr, 20.0, 4.0)


def test_table_fields():
    assert bootstrap.BOOT_DTYPE.names == ("label", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "kt_index0",
                                          "lo_index", "hi_index", "status", "kt0", "kt_lo", "kt_hi", "a0", "a_mean", "a_sd",
                                          "a_lo", "a_hi", "height0", "height_lo", "height_hi")
    import scarplet_amd as sl
    assert sl.bootstrap_segments is bootstrap.bootstrap_segments and hasattr(sl.Matcher, "bootstrap_segments")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_boot_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_segment_boot, _lib.SEGMENT_BOOT_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_segment_boot));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_segment_boot, %s));\n' % f for f in names)
    prog = tmp_path / "boot.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d\\n", SC_BOOT_MAX_REPLICATES, SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "boot"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [_lib.BOOT_MAX_REPLICATES, 11, 10]
    assert ctypes.sizeof(S) == 104 and dt.itemsize == 104 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert names == ["label", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "kt_index0", "lo_index",
                     "hi_index", "status", "kt0", "kt_lo", "kt_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi"]
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


BOOT_CALLS = ("sc_bootstrap_segments", "sc_bootstrap_segments_dem")


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in BOOT_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert len(_lib.SIGNATURES[n][1]) == 27 + (3 if n.endswith("_dem") else 0)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in BOOT_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_bootstrap.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)


def test_bootstrap_kernels_fit_their_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_bootstrap.hip")
    for k in ("k_bs_terms", "k_bs_reps", "k_bs_summary"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD
    # stage one stays where it was, with its budget
    s = kernel_table("sc_segment.hip")
    for k in ("k_sg_partial<true>", "k_sg_partial<false>", "k_sg_shift<true>", "k_sg_shift<false>", "k_sg_rank"):
        assert k in s and s[k]["scratch"] == 0 and s[k]["vgpr"] + s[k]["agpr"] <= 128, (k, s.get(k))


# ---- the restatement on the noisy case of docs/segments.md ----------------------------------------------------------------
def test_restatement_on_the_noisy_case():
    """h = 100, w = 2, the default ages, blocks of 30 (about ten of the hundred cells each), R = 1000: replicate 0 is the
    joint fit - index 10 -, and the percentile interval holds index 10 and is no narrower than fit_segments' [10, 10]."""
    z, cells, theta = sr.noisy_case()
    row = br.bootstrap_segments(z, 1.0, cells, np.ones(100, dtype=int), theta, 100, 2, AGES, 30.0, 1000)[0]
    print({k: v for k, v in row.items() if k not in ("index", "a", "near", "terms")})
    assert row["n_cells"] == 100 and row["n_profiles"] == 100 and row["n_blocks"] == 11 and row["n_failed"] == 0
    assert row["kt_index0"] == 10 and abs(row["a0"] - 1.00135) <= 1e-5     # docs/segments.md: a = 1.00135
    assert row["status"] == 0 and row["lo_index"] <= 10 <= row["hi_index"]
    lo, hi = 10, 10                                                        # fit_segments on the same cells (test_segment_host)
    assert row["lo_index"] <= lo and row["hi_index"] >= hi
    assert row["hist"].sum() == 1000 and row["hist"][row["lo_index"]:row["hi_index"] + 1].sum() >= 950
    assert row["a_lo"] <= row["a0"] <= row["a_hi"] and row["a_sd"] > 0
    assert not row["near"].any()
    # replicate 0 is the pooled argmin: the sse curve through the same terms, Spp - Q_i
    T = row["terms"].sum(axis=0)
    assert int(np.argmax(T[:, 1] ** 2 / T[:, 0])) == 10
    # the ranks of the percentiles
    assert br.ranks(1000, 0.95) == (25, 974) and br.ranks(1, 0.95) == (0, 0) and br.ranks(100, 0.5) == (25, 74)
