"""Scarp-profile dating, on the CPU: argument validation of sl.fit_profiles before any device call, the
sc_profile_fit layout, the kernels' scratch budget, the numpy restatement (tests/profile_reference.py) on surfaces
with known answers, and the restatement's own noise floor (float64 lstsq against a longdouble Gram-Schmidt) on the
inputs of tests/test_gpu_profiles.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.special import erf

import profile_reference as pr
from scarplet_amd import _lib, _plan, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()


# ---- sl.fit_profiles validates before any device call ---------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import scarplet_amd.core as core

    def refuse(device):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "_context", refuse)


def test_fit_profiles_validates_without_a_device(no_device):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0)
    plane = np.zeros((40, 50), dtype=bool)
    bad = [
        (dict(data=np.zeros((40, 50))), "not a DEMGrid"),
        (dict(data=sl.DEMGrid.from_array(np.zeros((1, 50)), 1.0)), "one row"),
        (dict(cells=[2000]), "cell outside"),
        (dict(cells=[-1]), "negative cell"),
        (dict(cells=[1.5]), "float cells"),
        (dict(cells=([1, 2], [3])), "rows and cols of two lengths"),
        (dict(cells=([40], [0])), "row outside"),
        (dict(cells=([0], [50])), "col outside"),
        (dict(cells=plane[:, :10]), "bool plane of another shape"),
        (dict(cells=np.zeros((2, 2), dtype=int)), "2-D indices"),
        (dict(angle=np.nan), "angle NaN"),
        (dict(angle=[0.1, 0.2, 0.3]), "three angles for two cells"),
        (dict(angle=np.zeros((40, 49))), "angle plane of another shape"),
        (dict(angle=[0.1, np.inf]), "angle inf"),
        (dict(angle="east"), "angle not a number"),
        (dict(half_length=3.0), "half_length of one cell"),
        (dict(half_length=np.nan), "half_length NaN"),
        (dict(half_length=-20.0), "half_length < 0"),
        (dict(half_length=2.0 * 1025), "more than 1024 cells"),
        (dict(swath=-1.0), "swath < 0"),
        (dict(swath=2.0 * 33), "swath of more than 32 cells"),
        (dict(ages=[]), "no age"),
        (dict(ages=[1.0, 1.0]), "ages not increasing"),
        (dict(ages=[0.0, 1.0]), "age 0"),
        (dict(ages=[1.0, np.nan]), "age NaN"),
        (dict(ages=[[1.0, 2.0]]), "2-D ages"),
        (dict(ages=np.arange(1.0, 66.0)), "65 ages"),
        (dict(delta=-0.5), "delta < 0"),
        (dict(delta=np.inf), "delta inf"),
        (dict(min_samples=1), "min_samples 1"),
        (dict(min_samples=11), "min_samples > h"),
        (dict(min_samples=4.5), "min_samples not an integer"),
        (dict(min_samples=True), "min_samples a bool"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_profiles(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device
    for kw in (dict(), dict(cells=plane), dict(cells=([1], [2]), angle=np.zeros((40, 50))), dict(cells=[], angle=0.0)):
        with pytest.raises(AssertionError, match="a device was asked for"):
            sl.fit_profiles(**dict(ok, **kw))


def test_check_args_normalises():
    from scarplet_amd import profiles
    plane = np.zeros((40, 50), dtype=bool)
    plane[3, 4] = plane[1, 7] = True
    ang = np.arange(2000.0).reshape(40, 50) * 1e-3
    idx, sa, ca, kt, h, w, de, d, ms = profiles.check_args((40, 50), 2.0, plane, ang, 21.9, 5.0, None, 1, 4)
    assert list(idx) == [57, 154] and idx.dtype == np.int64                # row-major order of the true cells
    assert np.array_equal(sa, np.sin(ang.ravel()[idx])) and np.array_equal(ca, np.cos(ang.ravel()[idx]))
    assert (h, w, de, d, ms) == (10, 2, 2.0, 1.0, 4) and np.array_equal(kt, AGES)
    idx = profiles.check_args((40, 50), 2.0, (np.array([3, 1]), np.array([4, 7])), 0.0, 20, 0, [5.0], 0, 2)[0]
    assert list(idx) == [154, 57]                                          # a (rows, cols) pair keeps its order


def test_fit_profiles_is_exported():
    import scarplet_amd as sl
    assert callable(sl.fit_profiles) and callable(sl.Matcher.fit_profiles)
    from scarplet_amd import profiles
    assert profiles.FIT_DTYPE.names == ("row", "col", "cell", "n", "kt_index", "lo_index", "hi_index", "status", "kt",
                                        "kt_lo", "kt_hi", "a", "b", "c0", "sse", "rmse", "height")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_profile_fit_layout_matches_c(tmp_path):
    names = [f for f, _ in _lib.sc_profile_fit._fields_]
    prog = tmp_path / "fit.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n'
                    '  printf("%zu\\n", sizeof(sc_profile_fit));\n'
                    + "".join('  printf("%%zu\\n", offsetof(sc_profile_fit, %s));\n' % f for f in names)
                    + '  printf("%d %d %d %d %d\\n", SC_PROFILE_MAX_AGES, SC_PROFILE_MAX_HALF, SC_PROFILE_MAX_SWATH, '
                      'SC_K_PROFILE, SC_K_COUNT);\n  printf("%d\\n", SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "fit"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.sc_profile_fit
    n = 1 + len(names)
    assert vals[:n] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
    assert _lib.PROFILE_DTYPE.itemsize == ctypes.sizeof(S) and _lib.PROFILE_DTYPE.names == tuple(names)
    assert vals[n:] == [_lib.PROFILE_MAX_AGES, _lib.PROFILE_MAX_HALF, _lib.PROFILE_MAX_SWATH, _lib.K_PROFILE,
                        len(_lib.K_NAMES), _lib.ABI_VERSION]
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile" and _lib.ABI_VERSION == 10


def test_library_exports_the_profile_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("sc_fit_profiles", "sc_fit_profiles_dem"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_kernel_name(_lib.K_PROFILE) == b"k_profile"


def test_profile_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_profile.hip")
    for k in ("k_pf_table", "k_pf_fit<true>", "k_pf_fit<false>"):
        assert k in t, sorted(t)
    for name, r in t.items():
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)                     # four waves per SIMD


# ---- the restatement on surfaces with known answers -------------------------------------------------------------------
def analytic(n, a, kt, de, amp=1.0, b=-0.01, c0=5.0, fine=1):
    """(z, centre cell) of c0 + b s + amp erf(s / (2 sqrt kt)), s measured from the centre cell along the profile
    of orientation a, on a grid ``fine`` times finer."""
    m = (n - 1) * fine + 1
    r, c = np.mgrid[0:m, 0:m].astype(np.float64)
    mid = (m - 1) // 2
    s = (de / fine) * ((c - mid) * np.cos(a) - (r - mid) * np.sin(a))
    return c0 + b * s + amp * erf(s / (2 * np.sqrt(kt))), mid * m + mid


@pytest.mark.parametrize("a", [0.0, np.pi / 2])
def test_noise_free_scarp_on_cell_centres(a):
    de, i_true = 2.0, 12
    z, cell = analytic(301, a, AGES[i_true], de)
    for h, w in ((100, 0), (30, 3)):
        row = pr.fit_profiles(z, de, [cell], a, h, w, AGES)[0]
        assert row["status"] == 0 and row["n"] == 2 * h + 1
        assert row["kt_index"] == i_true == row["lo_index"] == row["hi_index"]
        assert abs(row["a"] - 1.0) <= 1e-9 and abs(row["b"] + 0.01) <= 1e-9 and abs(row["c0"] - 5.0) <= 1e-9
        p = pr.sample_profile(z, *divmod(cell, 301), np.sin(a), np.cos(a), h, w)
        print("a %.3f h %d w %d: sse %.3g, variance %.3g" % (a, h, w, row["sse"], p.var()))
        assert row["sse"] <= 1e-18 * p.var()


@pytest.mark.parametrize("a", [0.2, -np.pi / 4])
def test_noise_free_scarp_oblique(a):
    """Off the cell centres bilinear interpolation of a smooth surface leaves an error of its own: the restatement on
    the grid and on a four times finer one, the difference recorded (it is the definition's, not a defect)."""
    de, i_true, h = 2.0, 12, 60
    rows = []
    for fine in (1, 4):
        z, cell = analytic(201, a, AGES[i_true], de, fine=fine)
        rows.append(pr.fit_profiles(z, de / fine, [cell], a, h * fine, 0, AGES)[0])
        assert rows[-1]["kt_index"] == i_true and rows[-1]["status"] == 0
    for f, true in (("a", 1.0), ("b", -0.01), ("c0", 5.0)):
        print("a %.3f %s: grid %.3e, 4 x finer %.3e off the truth" % (a, f, rows[0][f] - true, rows[1][f] - true))
        assert abs(rows[1][f] - true) <= abs(rows[0][f] - true) + 1e-12     # finer is no worse
        assert abs(rows[0][f] - true) <= 1e-2
    print("rmse: grid %.3e, 4 x finer %.3e" % (rows[0]["rmse"], rows[1]["rmse"]))


def test_noisy_synthetic_scarp_finds_its_age():
    z = pr.synthetic_z(600)                                                # kt0 = 10: index 10 of the default grid
    cells = pr.scarp_cells(600, 40, np.random.default_rng(3))
    for h, w in ((100, 0), (100, 5), (30, 5), (15, 2)):
        rows = pr.fit_profiles(z, 1.0, cells, 0.2, h, w, AGES)
        idx = np.array([r["kt_index"] for r in rows])
        a = np.array([r["a"] for r in rows])
        b = np.array([r["b"] for r in rows])
        print("h %d w %d: median index %g, range %d..%d; a %.4f..%.4f, b %.5f..%.5f (medians %.4f, %.5f)"
              % (h, w, np.median(idx), idx.min(), idx.max(), a.min(), a.max(), b.min(), b.max(), np.median(a), np.median(b)))
        assert np.median(idx) == 10
        assert np.all(a > 0)                                                # the direction convention: s runs uphill
        if h == 100:
            assert abs(np.median(a) - 1.0) <= 0.01 and abs(np.median(b) + 0.01) <= 5e-4
        assert all(r["lo_index"] <= r["kt_index"] <= r["hi_index"] for r in rows)


def test_too_few_points_and_interval_flags():
    z = pr.synthetic_z(64)
    ages = AGES[:12]
    row = pr.fit_profiles(z, 1.0, [0], 0.0, 20, 0, ages, min_samples=4)[0]        # the corner: nothing left of it
    assert row["status"] == 1 and row["kt_index"] == -1 and row["n"] == 21 and np.isnan(row["sse"])
    row = pr.fit_profiles(z, 1.0, [3], 0.0, 20, 0, ages, min_samples=4)[0]        # three points to the left
    assert row["status"] == 1 and row["n"] == 24
    row = pr.fit_profiles(z, 1.0, [4], 0.0, 20, 0, ages, min_samples=4)[0]
    assert row["status"] != 1 and row["n"] == 25
    assert pr.choose(np.array([1.0, 1.05, 2.0]), 13, 1.0) == (0, 0, 1, 2)
    assert pr.choose(np.array([3.0, 1.05, 1.0]), 13, 1.0) == (2, 1, 2, 4)
    assert pr.choose(np.array([1.0, 1.0, 1.0]), 13, 0.0) == (0, 0, 2, 6)          # ties: the smallest index wins


# ---- the noise floor the GPU tolerances stand on ------------------------------------------------------------------------
@pytest.mark.slow
def test_float64_restatement_against_longdouble_on_the_gpu_inputs():
    """Two CPU solutions of the same fits - LAPACK's lstsq in float64 and Gram-Schmidt in longdouble - on every input
    tests/test_gpu_profiles.py compares: their differences are the reference's own error.  compare_rows holds them to
    the tolerances the device is held to (1e-9; at most 1 % of a case decided inside it); the figures are printed."""
    worst = {"sse": 0.0, "coef": 0.0, "cond": 0.0, "ties": 0}
    for case in pr.gpu_cases():
        idx, ref = pr.restate(case)
        _, ld = pr.restate(case, fit=pr.fit_age_longdouble)
        st = pr.compare_rows(ref, ld, case["h"], case["de"], case["delta"])
        print("%-22s %s" % (case["name"], st))
        for k in worst:
            worst[k] = max(worst[k], st[k])
    print("worst over the cases:", worst)
    assert worst["cond"] <= pr.COND_MAX
