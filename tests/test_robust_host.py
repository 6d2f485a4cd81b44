"""Weights and robust fits of sl.fit_profiles on the CPU: argument validation before the library is loaded, the layout of
sc_profile_robust_fit and the header's ABI, the exported symbols, the kernels' register budget, the restatement's own
noise floor (tests/robust_reference.py: float64 lstsq against a longdouble Gram-Schmidt) on the inputs of
tests/test_gpu_robust.py, and what the feature is for: the pit surface of docs/profiles.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import robust_reference as rr
from scarplet_amd import _lib, profiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ("loss", "scale", "n_down", "ls_index")


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
    ok = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0, robust="huber")
    plane = np.ones((40, 50))
    bad = [
        (dict(robust="cauchy"), "a loss that is not built"),
        (dict(robust="Huber"), "the names are lower case"),
        (dict(robust=1), "robust not a string"),
        (dict(robust=True), "robust a bool"),
        (dict(tuning=0.0), "tuning 0"),
        (dict(tuning=-1.0), "tuning < 0"),
        (dict(tuning=np.nan), "tuning NaN"),
        (dict(tuning=np.inf), "tuning inf"),
        (dict(tuning="wide"), "tuning not a number"),
        (dict(tuning=True), "tuning a bool"),
        (dict(iterations=0), "iterations < 1"),
        (dict(iterations=65), "iterations > 64"),
        (dict(iterations=8.0), "iterations not an integer"),
        (dict(iterations=True), "iterations a bool"),
        (dict(robust_scale=0.0), "robust_scale 0"),
        (dict(robust_scale=-0.1), "robust_scale < 0"),
        (dict(robust_scale=np.nan), "robust_scale NaN"),
        (dict(robust_scale=np.inf), "robust_scale inf"),
        (dict(weights=np.ones((40, 51))), "a plane of another shape"),
        (dict(weights=np.ones(2000)), "a plane that is none"),
        (dict(weights=-plane), "weights < 0"),
        (dict(weights=np.where(np.arange(2000).reshape(40, 50) == 7, np.inf, 1.0)), "an infinite weight"),
        (dict(weights="heavy"), "weights not numbers"),
        (dict(max_shift=4.0), "robust with max_shift"),
        (dict(robust=None, weights=plane, max_shift=4.0), "weights with max_shift"),
        (dict(robust=None, tuning=2.0), "tuning without robust"),
        (dict(robust=None, robust_scale=0.1), "robust_scale without robust"),
        (dict(robust=None, weights=plane, tuning=2.0), "tuning with weights alone"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_profiles(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device
    for kw in (dict(), dict(robust="tukey"), dict(tuning=2.5), dict(iterations=1), dict(iterations=64), dict(robust_scale=0.3),
               dict(weights=plane), dict(robust=None, weights=plane), dict(weights=np.where(plane > 0, np.nan, 1.0)),
               dict(weights=0 * plane), dict(return_curve=True), dict(robust=None, iterations=3), dict(cells=[])):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_profiles(**dict(ok, **kw))


def test_matcher_route_validates():
    import scarplet_amd as sl

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    for kw in (dict(robust="cauchy"), dict(robust="huber", tuning=0.0), dict(robust="tukey", iterations=0),
               dict(robust="huber", robust_scale=-1.0), dict(weights=np.ones((4, 5))), dict(robust="huber", max_shift=2.0)):
        with pytest.raises(ValueError):
            sl.Matcher.fit_profiles(Held(), [3, 77], 20.0, angle=0.1, **kw)


def test_check_robust_normalises():
    assert profiles.check_robust((40, 50), None, None, None, 8, None, None) is None
    assert profiles.check_robust((40, 50), None, None, None, 8, None, 4.0) is None        # max_shift alone is the parent's call
    assert profiles.check_robust((40, 50), None, "huber", None, 8, None, None) == (None, _lib.ROBUST_HUBER, 1.345, 8, 0.0)
    assert profiles.check_robust((40, 50), None, "tukey", None, 3, 0.5, None) == (None, _lib.ROBUST_TUKEY, 4.685, 3, 0.5)
    plane, loss, k, T, sigma = profiles.check_robust((40, 50), np.ones((40, 50), dtype=np.float32), None, None, 8, None, None)
    assert plane.dtype == np.float64 and plane.flags.c_contiguous and (loss, sigma) == (_lib.ROBUST_NONE, 0.0)


def test_table_fields_and_defaults():
    names = profiles.ROBUST_FIT_DTYPE.names
    assert names[:len(profiles.FIT_DTYPE.names)] == profiles.FIT_DTYPE.names and names[-4:] == NEW_FIELDS
    t = profiles._table(np.zeros(2, dtype=_lib.PROFILE_ROBUST_DTYPE), 50, label=np.array([4, 9]))
    assert t.dtype.names == names + ("label",) and t["label"].tolist() == [4, 9]
    assert profiles._table(np.zeros(2, dtype=_lib.PROFILE_DTYPE), 50).dtype == profiles.FIT_DTYPE      # the parent's table
    import inspect
    import scarplet_amd as sl
    for f in (sl.fit_profiles, sl.Matcher.fit_profiles):
        p = inspect.signature(f).parameters
        assert [p[k].default for k in ("weights", "robust", "tuning", "iterations", "robust_scale")] == [None, None, None, 8, None]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_robust_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_profile_robust_fit, _lib.PROFILE_ROBUST_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_profile_robust_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_profile_robust_fit, %s));\n' % f for f in names)
    prog = tmp_path / "robust.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d %d %d %d\\n", SC_K_COUNT, SC_ABI_VERSION, SC_ROBUST_NONE, SC_ROBUST_HUBER,'
                    ' SC_ROBUST_TUKEY, SC_ROBUST_MAX_ITER);\n  return 0;\n}\n')
    exe = tmp_path / "robust"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [11, 10, 0, 1, 2, 64]
    assert ctypes.sizeof(S) == 120 and dt.itemsize == 120 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    # the parent's row is this row's head
    P = _lib.sc_profile_fit
    assert names[:len(P._fields_)] == [f for f, _ in P._fields_] and tuple(names[len(P._fields_):]) == NEW_FIELDS
    assert all(getattr(S, f).offset == getattr(P, f).offset for f, _ in P._fields_)
    assert (_lib.ROBUST_NONE, _lib.ROBUST_HUBER, _lib.ROBUST_TUKEY, _lib.ROBUST_MAX_ITER) == (0, 1, 2, 64)
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


ROBUST_CALLS = ("sc_fit_profiles_robust", "sc_fit_profiles_robust_dem")


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in ROBUST_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert len(_lib.SIGNATURES[n][1]) == 19 + (3 if n.endswith("_dem") else 0)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ROBUST_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_robust.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    assert "sc_fit.h" in re.search(r"^HDR\s*=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_robust_kernels_fit_their_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_robust.hip")
    fits = [k for k in t if k.startswith("k_rb_fit<")]
    assert len(fits) == 12, sorted(t)                                      # table in LDS or not, a weight plane or not, three losses
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)                        # four waves per SIMD


def test_the_kernels_use_no_inline_assembly():
    for f in ("sc_robust.hip", "sc_fit.h"):
        txt = open(os.path.join(ROOT, "scarplet_amd", "csrc", f)).read()
        assert not re.search(r"\basm\b|__asm", txt), f


# ---- the restatement itself ------------------------------------------------------------------------------------------------------
def test_order_statistic_and_factors():
    """rank (n - 1) // 2 of np.sort is the lower median; f and rho at, below and beyond c."""
    for n in (4, 5, 63, 64, 65):
        x = np.random.default_rng(n).permutation(n).astype(np.float64)
        assert np.sort(x)[(n - 1) // 2] == float((n - 1) // 2)
    r = np.array([0.0, 0.5, -1.0, 2.0, -4.0])
    assert np.array_equal(rr.factor("huber", r, 1.0), [1.0, 1.0, 1.0, 0.5, 0.25])
    assert np.array_equal(rr.rho("huber", r, 1.0), [0.0, 0.25, 1.0, 3.0, 7.0])
    assert np.array_equal(rr.factor("tukey", r, 2.0), [1.0, (1 - 0.0625) ** 2, 0.5625, 0.0, 0.0])
    assert np.allclose(rr.rho("tukey", r, 2.0), [0.0, (4 / 3) * (1 - (1 - 0.0625) ** 3), (4 / 3) * (1 - 0.75 ** 3), 4 / 3, 4 / 3], rtol=1e-15)
    # rho'(r) = 2 r f(r): the weights are those of the loss
    for loss in ("huber", "tukey"):
        x, d = np.linspace(-3, 3, 61) + 0.013, 1e-6
        num = (rr.rho(loss, x + d, 1.7) - rr.rho(loss, x - d, 1.7)) / (2 * d)
        assert np.allclose(num, 2 * x * rr.factor(loss, x, 1.7), atol=1e-8)


def test_weights_of_one_and_a_far_constant_are_the_plain_fit():
    import profile_reference as pr
    z = pr.synthetic_z(300, seed=7)
    cells = pr.scarp_cells(300, 6, np.random.default_rng(1), spread=2.0)
    ages = np.array([3.0, 10.0, 30.0])
    plain = pr.fit_profiles(z, 1.0, cells, 0.2, 40, 2, ages, min_samples=10)
    ones = rr.fit_profiles(z, np.ones(z.shape), 1.0, cells, 0.2, 40, 2, ages, min_samples=10)
    far = rr.fit_profiles(z, None, 1.0, cells, 0.2, 40, 2, ages, min_samples=10, robust="huber", tuning=1e6)
    for p, o, f in zip(plain, ones, far):
        assert p["n"] == o["n"] == f["n"] and p["kt_index"] == o["kt_index"] == f["kt_index"] == f["ls_index"]
        assert abs(o["sse"] - p["sse"]) <= 1e-11 * p["sse"] and abs(f["loss"] - p["sse"]) <= 1e-11 * p["sse"]
        assert f["n_down"] == 0 and f["scale"] > 0 and np.isnan(o["scale"])


# ---- the noise floor the GPU tolerance stands on --------------------------------------------------------------------------------
FLOOR = rr.RTOL / 100


@pytest.mark.slow
@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_float64_restatement_against_longdouble_on_the_gpu_inputs(loss):
    """Two CPU solutions of the same fits - LAPACK's lstsq in float64 and weighted Gram-Schmidt in longdouble, each run
    through all the iterates on its own - on every input tests/test_gpu_robust.py compares, by compare_rows: their
    difference is the reference's own error, and it must stay a hundred times below the tolerance the device is held
    to.  Measured: loss and curve 2.8e-12, scale 3.4e-12 (both on the Carrizo crop, elevations of hundreds of metres over
    a range of a few), coefficients over the range 9.1e-12 (the "NaN cells" case), no index, no n_down and no dead age
    decided differently."""
    worst = {"loss": 0.0, "coef": 0.0, "scale": 0.0, "cond": 0.0, "ties": 0}
    for name, c in rr.gpu_cases(loss).items():
        ref = rr.restate(c)
        ld = rr.restate(c, fit=rr.wfit_longdouble)
        st = rr.compare_rows(c, ref, ld)
        print("%-6s %-28s %s" % (loss, name, st))
        for k in worst:
            worst[k] = max(worst[k], st[k])
    print("worst over the cases:", worst)
    assert worst["cond"] <= rr.COND_MAX and worst["ties"] == 0
    assert worst["loss"] <= FLOOR and worst["coef"] <= FLOOR and worst["scale"] <= FLOOR


# ---- what the feature is for ------------------------------------------------------------------------------------------------------
def test_robust_fits_find_the_age_the_pits_hide():
    """synthetic_scarp(600) with 400 Gaussian pits (robust_reference.pit_surface: seed 20261019), 100 cells on the scarp
    line, h = 100, w = 2, the default 35 ages, T = 8: the share of cells whose best age is the true one (index 10).
    Least squares 58, Huber 76, Tukey 80 - each robust loss at least 5 cells of 100 ahead."""
    share = {}
    for loss in (None, "huber", "tukey"):
        c = rr.pit_case(robust=loss)
        rows = rr.restate(c, cond=False)
        assert len(rows) == 100 and all(r["status"] & 1 == 0 for r in rows)
        share[loss] = rr.share_on(rows)
        if loss:
            assert rr.share_on([dict(kt_index=r["ls_index"]) for r in rows]) == share[None]      # ls_index is the plain fit's age
    print(share)
    assert share["huber"] >= share[None] + 5 and share["tukey"] >= share[None] + 5
