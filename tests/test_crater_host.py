"""The Crater template on the host (docs/craters.md): the numpy class against the reference's template() captured in
tests/golden/ref_crater.npz (tools/gen_crater_golden.py), the window-limit rectangle, what refuses what, and the
library's side as far as it shows without a GPU - the declared call, the build id, the kernels' register budgets."""
import ctypes
import os
import re

import numpy as np
import pytest

import scarplet_amd as sl
from scarplet_amd import _lib, WindowedTemplate as WT
from conftest import load_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(10, 1, 64, 64, 1), (10, 10, 65, 63, 1), (20, 3, 96, 80, 2), (6, 0.5, 33, 33, 1), (3, 1, 32, 32, 1),
         (40, 30, 128, 128, 1)]


def golden_cases():
    out = []
    for c in load_cases("ref_crater.npz"):
        out.append(((float(c["r"]), float(c["kt"]), int(c["nx"]), int(c["ny"]), float(c["de"])), np.asarray(c["W"])))
    return out


def test_golden_holds_the_six_cases():
    got = [args for args, _ in golden_cases()]
    assert got == [tuple(float(v) if k in (0, 1, 4) else v for k, v in enumerate(c)) for c in CASES]
    for (r, kt, nx, ny, de), W in golden_cases():
        assert W.shape == (ny, nx) and W.dtype == np.float64
        nz = np.abs(W[W != 0])
        assert 36 <= nz.size <= 556 and nz.min() >= 1e-9 * nz.max()       # the support is the masks', not a residue


@pytest.mark.parametrize("k", range(len(CASES)))
def test_numpy_template_is_the_reference(k):
    (r, kt, nx, ny, de), gold = golden_cases()[k]
    W = sl.Crater(r, kt, nx, ny, de).template()
    assert W.shape == gold.shape
    assert np.array_equal(W != 0, gold != 0), int(((W != 0) != (gold != 0)).sum())
    err = np.abs(W - gold).max() / np.abs(gold).max()
    print("case %d: %d cells, max |dW| / max |W| = %.2e" % (k, int((gold != 0).sum()), err))
    assert err <= 1e-13


@pytest.mark.parametrize("k", range(len(CASES)))
def test_support_box_holds_the_support(k):
    (r, kt, nx, ny, de), gold = golden_cases()[k]
    pmin, pmax, qmin, qmax = WT.crater_box(r / de, de)
    ii, jj = np.nonzero(gold)
    assert ny // 2 + pmin <= ii.min() and ii.max() <= ny // 2 + pmax
    assert nx // 2 + qmin <= jj.min() and jj.max() <= nx // 2 + qmax
    # ... and the ring bounds of the tables hold every cell of it
    t = WT.crater_tables([r], [kt], nx, ny, de)
    x, y = WT.centred_axis(nx, de), WT.centred_axis(ny, de)
    rho2 = x[jj] ** 2 + y[ii] ** 2
    assert (rho2 >= t["ring"][0, 0]).all() and (rho2 <= t["ring"][0, 1]).all()


@pytest.mark.parametrize("r,nx,ny,de", [(10, 64, 64, 1), (10, 65, 63, 1), (20, 96, 80, 2), (6, 33, 34, 1), (40, 60, 128, 1)])
def test_window_limits_are_the_rectangle(r, nx, ny, de):
    t = sl.Crater(r, 3.0, nx, ny, de)
    pmin, pmax, qmin, qmax = t._support_bbox()
    assert (pmin, pmax, qmin, qmax) == WT.crater_box(r / de, de)
    ilo, ihi, jlo, jhi = -pmin, ny - 1 - pmax, -qmin, nx - 1 - qmax
    assert WT.crater_limits((pmin, pmax, qmin, qmax), nx, ny) == (ilo, ihi, jlo, jhi)
    want = np.ones((ny, nx), dtype=bool)
    if ihi >= ilo and jhi >= jlo:
        want[ilo:ihi + 1, jlo:jhi + 1] = False
    lim = t.get_window_limits()
    assert lim.dtype == bool and np.array_equal(lim, want)
    if (r, nx) == (40, 60):
        assert lim.all()                                # a box wider than the grid: every cell masked
    else:
        assert not lim[ny // 2, nx // 2] and lim[0].all() and lim[:, -1].all()


def test_tables_are_the_reference_scalars():
    t = WT.crater_tables([10, 20], [1.0, 30.0], 128, 128, 2.0)
    th = np.linspace(0, 2 * np.pi, num=359, endpoint=False)
    assert t["theta_tab"].shape == (359, 3) and t["dxy"].shape == (2, 359, 2) and t["boxes"].shape == (2, 4)
    for k in (0, 1, 89, 90, 179, 180, 269, 270, 358):
        assert t["theta_tab"][k, 0] == np.cos(-th[k]) and t["theta_tab"][k, 1] == np.sin(-th[k])
        assert t["theta_tab"][k, 2] == (-1.0 if np.pi / 2 < th[k] < 3 * np.pi / 2 else 1.0)
        assert t["dxy"][1, k, 0] == (20 / 2.0) * np.cos(th[k]) and t["dxy"][1, k, 1] == (20 / 2.0) * np.sin(th[k])
    assert t["d_half"] == 5 / 2.0
    assert t["age_tab"][1, 0] == 2. * 30.0 ** (3 / 2.) * np.sqrt(np.pi) and t["age_tab"][1, 1] == 4. * 30.0
    assert set(t["theta_tab"][:, 2]) == {-1.0, 1.0}


def test_crater_is_exported_and_describes_nothing_to_the_device():
    assert sl.Crater is WT.Crater and callable(sl.match_craters) and hasattr(sl.Matcher, "search_craters")
    assert not hasattr(sl.Crater, "_device_descriptor")
    assert WT.builtin_twin(sl.Crater) is None


def test_match_refuses_crater_and_names_match_craters():
    g = sl.DEMGrid.from_array(np.zeros((64, 64)), 1.0)
    for call in (lambda: sl.match(g, sl.Crater, scale=10, age=10.),
                 lambda: sl.match(g, sl.Crater, scale=10),
                 lambda: sl.match_template(g, sl.Crater, 10, 10., 0.),
                 lambda: sl.calculate_best_fit_parameters(g, sl.Crater, 10, 10.)):
        with pytest.raises(TypeError, match="match_craters"):
            call()


def test_a_radius_too_large_for_the_grid_is_a_value_error():
    g = sl.DEMGrid.from_array(np.zeros((64, 64)), 1.0)
    with pytest.raises(ValueError, match="leaves the 64 x 64 grid"):
        sl.match_craters(g, [6, 40])
    with pytest.raises(ValueError):
        WT.crater_tables([10], [1.0], 28, 200, 1.0)         # columns 14 - 14 .. 14 + 14: one beyond the last
    WT.crater_tables([10], [1.0], 29, 200, 1.0)
    with pytest.raises(ValueError):
        sl.match_craters(g, [6], ages=[0.0])


# ---- the library's side ------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint sc_crater_windows\s*\(", code)
    assert len(_lib.SIGNATURES["sc_crater_windows"][1]) == 14
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


def test_library_exports_the_call():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sc_crater_windows")
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_crater.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)


def test_crater_kernels_fit_their_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_crater.hip")
    for k in ("k_crater_window", "k_crater_sums"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD
