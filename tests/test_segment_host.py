"""One age per trace segment, on the CPU: the numpy restatement (tests/segment_reference.py) on surfaces with known
answers and on the noisy surface of docs/segments.md, argument validation of sl.fit_segments before any device call,
the struct layouts, the exports and the kernels' register and scratch budget."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import profile_reference as pr
import segment_reference as sr
from scarplet_amd import _lib, _plan
from test_profile_host import analytic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()


# ---- the restatement on surfaces with known answers -------------------------------------------------------------------
def test_noise_free_surface_recovers_every_coefficient():
    """c0 + b s + erf(s / (2 sqrt kt)) with s measured from the centre cell along the profile of orientation 0: a
    cell d columns from the centre sees s + d de, so its own intercept is c0 + b d de and the shared erf is centred
    only at d = 0 - the cells of this segment lie on the centre COLUMN, where every profile is centred, and the ramp
    along the rows is added by hand: an intercept and a slope per profile, one amplitude, one age."""
    de, i_true, n = 2.0, 12, 301
    z, cell = analytic(n, 0.0, AGES[i_true], de, amp=1.5)
    mid = (n - 1) // 2
    rows = np.arange(mid - 20, mid + 21, 4)
    tilt = 0.02 * (rows - mid)                                            # per-row intercept
    slope = 1e-3 * (rows - mid)                                           # per-row far-field slope
    s = de * (np.arange(n) - mid)
    z = z.copy()
    z[rows] += tilt[:, None] + slope[:, None] * s[None, :]
    cells = rows * n + mid
    for h, w in ((100, 0), (30, 0)):
        row = sr.fit_segments(z, de, cells, np.full(len(cells), 3), 0.0, h, w, AGES)[0]
        assert row["label"] == 3 and row["status"] == 0 and row["n_profiles"] == len(cells) == row["n_cells"]
        assert row["n"] == len(cells) * (2 * h + 1) and row["dof"] == row["n"] - 2 * len(cells) - 1
        assert row["kt_index"] == i_true == row["lo_index"] == row["hi_index"]
        coef = row["coefs"][i_true]
        assert abs(row["a"] - 1.5) <= 1e-9 and coef[-1] == row["a"]
        assert np.max(np.abs(coef[0:-1:2] - (5.0 + tilt))) <= 1e-9
        assert np.max(np.abs(coef[1:-1:2] - (-0.01 + slope))) <= 1e-9
        assert row["sse"] <= 1e-18 * row["n"]


def test_one_profile_is_the_single_cell_fit():
    z = pr.synthetic_z(300, seed=3)
    cells = pr.scarp_cells(300, 5, np.random.default_rng(1))
    seg = sr.fit_segments(z, 1.0, cells, np.arange(1, 6), 0.2, 60, 2, AGES)
    one = pr.fit_profiles(z, 1.0, cells, 0.2, 60, 2, AGES)
    for s, o in zip(seg, one):
        assert s["dof"] == o["n"] - 3 and s["n_profiles"] == 1
        assert (s["kt_index"], s["lo_index"], s["hi_index"], s["status"]) == (o["kt_index"], o["lo_index"], o["hi_index"], o["status"])
        assert abs(s["a"] - o["a"]) <= 1e-12 and abs(s["sse"] - o["sse"]) <= 1e-12 * o["sse"]


def test_restatement_against_the_orthogonalised_form():
    """The device's algebra written in numpy - per-profile orthogonalisation, a = sum Sep / sum See - against the
    full-matrix lstsq on clipped profiles with NaN cells: the two agree far inside the GPU tolerance."""
    z = pr.synthetic_z(200, seed=5, sigma=0.2).copy()
    z[np.random.default_rng(2).random(z.shape) < 0.01] = np.nan
    cells = pr.scarp_cells(200, 30, np.random.default_rng(4), spread=2.0)
    ang = 0.2 + 0.05 * np.random.default_rng(6).standard_normal(30)
    h, w, ms = 80, 1, 10
    row = sr.fit_segments(z, 1.0, cells, np.ones(30, dtype=int), ang, h, w, AGES[:24], min_samples=ms)[0]
    assert row["status"] != 1 and 0 < row["n_profiles"] <= 30 and row["n"] < row["n_profiles"] * (2 * h + 1)
    from scipy.special import erf
    j = np.arange(-h, h + 1)
    worst_a = worst_s = 0.0
    for i, kt in enumerate(AGES[:24]):
        See = Sep = 0.0
        parts = []
        for k, cell in enumerate(cells):
            p = pr.sample_profile(z, float(cell // 200), float(cell % 200), np.sin(ang[k]), np.cos(ang[k]), h, w)
            ok = ~np.isnan(p)
            if (ok & (j < 0)).sum() < ms or (ok & (j > 0)).sum() < ms:
                continue
            s, pv = j[ok].astype(float), p[ok]
            e = erf(s / (2 * np.sqrt(kt)))
            sc = s - s.mean()
            beta, gamma = (sc * (pv - pv.mean())).sum() / (sc * sc).sum(), (sc * (e - e.mean())).sum() / (sc * sc).sum()
            e2, p2 = (e - e.mean()) - gamma * sc, (pv - pv.mean()) - beta * sc
            See, Sep = See + (e2 * e2).sum(), Sep + (e2 * p2).sum()
            parts.append((p2, e2))
        a = Sep / See
        sse = sum(((p2 - a * e2) ** 2).sum() for p2, e2 in parts)
        worst_a = max(worst_a, abs(a - row["coefs"][i][-1]))
        worst_s = max(worst_s, abs(sse - row["curve"][i]) / row["curve"][i])
    print("orthogonalised against lstsq: a %.2e, sse %.2e relative; condition number %.1f" % (worst_a, worst_s, row["cond"]))
    assert worst_a <= 1e-11 and worst_s <= 1e-11 and row["cond"] <= pr.COND_MAX


def test_noisy_surface_joint_fit_finds_what_single_cells_do_not():
    """The figures of docs/segments.md: synthetic_scarp(600, sigma=0.5), 100 cells on the line, h = 100, w = 2."""
    z, cells, theta = sr.noisy_case()
    assert len(cells) == 100
    row = sr.fit_segments(z, 1.0, cells, np.ones(100, dtype=int), theta, 100, 2, AGES)[0]
    single = pr.fit_profiles(z, 1.0, cells, theta, 100, 2, AGES)
    idx = np.array([r["kt_index"] for r in single])
    print("joint: index %d, interval [%d, %d], a %.5f, condition number %.1f; single cells: %d of 100 on index 10, %d..%d"
          % (row["kt_index"], row["lo_index"], row["hi_index"], row["a"], row["cond"], (idx == 10).sum(), idx.min(), idx.max()))
    assert row["kt_index"] == 10 and row["lo_index"] == 10 and row["hi_index"] == 10
    assert abs(row["a"] - 1.00135) <= 5e-5
    assert (idx == 10).sum() <= 30


def test_unusable_cells_and_min_profiles():
    z = pr.synthetic_z(64)
    ages = AGES[:12]
    cells = np.array([0, 3, 30 * 64 + 30, 31 * 64 + 30])                  # two at the border without a left side
    row = sr.fit_segments(z, 1.0, cells, [7, 7, 7, 7], 0.0, 20, 0, ages)[0]
    assert list(row["used"]) == [0, 0, 1, 1] and row["n_cells"] == 4 and row["n_profiles"] == 2 and row["status"] != 1
    assert row["n"] == 82 and row["dof"] == 77
    row = sr.fit_segments(z, 1.0, cells, [7, 7, 7, 7], 0.0, 20, 0, ages, min_profiles=3)[0]
    assert row["status"] == 1 and row["kt_index"] == -1 and np.isnan(row["a"]) and row["n_profiles"] == 2
    rows = sr.fit_segments(z, 1.0, cells, [2, 0, 1, -4], 0.0, 20, 0, ages)          # labels <= 0 are dropped
    assert [r["label"] for r in rows] == [1, 2] and rows[1]["status"] == 1 and rows[1]["n_profiles"] == 0
    assert rows[1]["n"] == 0 and rows[1]["dof"] == -1


# ---- sl.fit_segments validates before any device call -----------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import scarplet_amd.core as core

    def refuse(device):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "_context", refuse)


def test_fit_segments_validates_without_a_device(no_device):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77], labels=[1, 1], angle=0.1, half_length=20.0)
    bad = [
        (dict(data=np.zeros((40, 50))), "not a DEMGrid"),
        (dict(cells=[2000]), "cell outside"),
        (dict(cells=[1.5, 2.5]), "float cells"),
        (dict(angle=np.nan), "angle NaN"),
        (dict(angle=[0.1, 0.2, 0.3]), "three angles for two cells"),
        (dict(half_length=3.0), "half_length of one cell"),
        (dict(half_length=2.0 * 1025), "more than 1024 cells"),
        (dict(swath=2.0 * 33), "swath of more than 32 cells"),
        (dict(ages=[1.0, 1.0]), "ages not increasing"),
        (dict(ages=np.arange(1.0, 66.0)), "65 ages"),
        (dict(delta=-0.5), "delta < 0"),
        (dict(min_samples=1), "min_samples 1"),
        (dict(min_samples=11), "min_samples > h"),
        (dict(labels=[1]), "one label for two cells"),
        (dict(labels=[1.0, 2.0]), "float labels"),
        (dict(labels=[True, True]), "bool labels"),
        (dict(labels=np.ones((40, 49), dtype=int)), "label plane of another shape"),
        (dict(labels=np.ones((2, 1, 1), dtype=int)), "3-D labels"),
        (dict(labels=[1, 2 ** 31]), "a label beyond 32 bits"),
        (dict(labels="ab"), "labels not numbers"),
        (dict(min_profiles=0), "min_profiles 0"),
        (dict(min_profiles=1.5), "min_profiles not an integer"),
        (dict(min_profiles=True), "min_profiles a bool"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_segments(**dict(ok, **kw))
            pytest.fail(what)
    plane = np.zeros((40, 50), dtype=np.int32)
    plane[0, 3] = plane[1, 27] = 4
    for kw in (dict(), dict(labels=plane), dict(labels=[0, -1]), dict(cells=[], labels=[], angle=0.0),
               dict(cells=plane > 0, labels=plane, angle=np.zeros((40, 50)))):
        with pytest.raises(AssertionError, match="a device was asked for"):
            sl.fit_segments(**dict(ok, **kw))


def test_matcher_route_validates_its_own_arguments():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 4, 5, 1.0
    tr = traces.Traces(np.zeros((4, 5), dtype=bool), np.zeros((4, 5), dtype=np.int32), traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    with pytest.raises(ValueError, match="strike"):
        sl.Matcher.fit_segments(Held(), tr, 2.0, strike="trace")
    with pytest.raises(ValueError, match="Traces"):
        sl.Matcher.fit_segments(Held(), np.zeros((4, 5)), 2.0)
    Held.whole = False
    with pytest.raises(ValueError, match="whole DEM"):
        sl.Matcher.fit_segments(Held(), tr, 2.0)


def test_check_args_groups_by_label():
    from scarplet_amd import segments
    ang = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    out = segments.check_args((40, 50), 2.0, [10, 11, 12, 13, 14, 15], [5, 2, 0, 5, 2, 9], ang, 21.9, 5.0, None, 1, 4, 2)
    idx, sa, ca, seg_start, seg_label, kt, h, w, de, d, ms, mp, order, kept = out
    assert list(idx) == [11, 14, 10, 13, 15] and idx.dtype == np.int64     # a stable sort: input order within a label
    assert np.array_equal(sa, np.sin(ang[[1, 4, 0, 3, 5]])) and np.array_equal(ca, np.cos(ang[[1, 4, 0, 3, 5]]))
    assert list(seg_start) == [0, 2, 4, 5] and seg_start.dtype == np.int64
    assert list(seg_label) == [2, 5, 9] and seg_label.dtype == np.int32
    assert (h, w, de, d, ms, mp) == (10, 2, 2.0, 1.0, 4, 2) and np.array_equal(kt, AGES)
    assert list(kept) == [0, 1, 3, 4, 5] and list(kept[order]) == [1, 4, 0, 3, 5]


def test_fit_segments_is_exported():
    import scarplet_amd as sl
    assert callable(sl.fit_segments) and callable(sl.Matcher.fit_segments)
    from scarplet_amd import segments
    assert segments.FIT_DTYPE.names == ("label", "n_cells", "n_profiles", "n", "dof", "kt_index", "lo_index", "hi_index",
                                        "status", "kt", "kt_lo", "kt_hi", "a", "sse", "rmse", "height")
    assert segments.CELL_DTYPE.names == ("row", "col", "cell", "used", "n", "b", "c0", "sse", "label")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_segment_struct_layouts_match_c(tmp_path):
    structs = [("sc_segment_fit", _lib.sc_segment_fit, _lib.SEGMENT_FIT_DTYPE),
               ("sc_segment_cell", _lib.sc_segment_cell, _lib.SEGMENT_CELL_DTYPE)]
    body = ""
    for cname, S, _ in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f, _ in S._fields_)
    prog = tmp_path / "seg.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%lld %d %d\\n", (long long)SC_SEGMENT_MAX_PARK, SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "seg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, S, dt in structs:
        names = [f for f, _ in S._fields_]
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
        assert dt.itemsize == ctypes.sizeof(S) and dt.names == tuple(names)
    assert vals == want + [_lib.SEGMENT_MAX_PARK, len(_lib.K_NAMES), 10]   # no new timing slot, the ABI as it was
    assert [f for f, _ in _lib.sc_segment_fit._fields_] == ["label", "n_cells", "n_profiles", "n", "dof", "kt_index", "lo_index",
                                                           "hi_index", "status", "kt", "kt_lo", "kt_hi", "a", "sse", "rmse"]
    assert [f for f, _ in _lib.sc_segment_cell._fields_] == ["cell", "used", "n", "b", "c0", "sse"]


def test_header_still_says_abi_10():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert "SC_K_SEGMENT" not in txt


def test_library_exports_the_segment_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("sc_fit_segments", "sc_fit_segments_dem"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_segment_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_segment.hip")
    for k in ("k_sg_partial<true>", "k_sg_partial<false>", "k_sg_rank", "k_sg_sum1<2>", "k_sg_sum1<1>", "k_sg_sum2<2>",
              "k_sg_sum2<1>", "k_sg_resid<true>", "k_sg_resid<false>", "k_sg_choose<sc_segment_cell>"):
        assert k in t, sorted(t)
    for name, r in t.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)                     # four waves per SIMD
