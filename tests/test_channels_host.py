"""sl.fit_channels (docs/channels.md) on the CPU: argument validation before the library is loaded, the table's fields, the
binding against its SIGNATURES entry through a recording fake library, the header's constants and ABI, the kernels' scratch
budget, the two numpy restatements (tests/channel_reference.py) against each other on every input of
tests/test_gpu_channels.py, and what the model recovers on a 2-D surface and against the Channel search."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import channel_reference as cr
from scarplet_amd import _lib
from test_fit_binding_host import fake_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 8.0, 6))


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_fit_channels_validates_before_the_library_is_loaded(no_library):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0, frequencies=FS)  # h = 10, min_samples = 4
    bad = [
        (dict(frequencies=[]), "no frequency"),
        (dict(frequencies=None), "frequencies None"),
        (dict(frequencies="high"), "frequencies no numbers"),
        (dict(frequencies=[[0.01, 0.02]]), "frequencies 2-D"),
        (dict(frequencies=[0.01, np.nan]), "a NaN frequency"),
        (dict(frequencies=[0.01, np.inf]), "an infinite frequency"),
        (dict(frequencies=[0.0, 0.01]), "a frequency of 0"),
        (dict(frequencies=[-0.01, 0.01]), "a negative frequency"),
        (dict(frequencies=[0.02, 0.01]), "descending frequencies"),
        (dict(frequencies=[0.01, 0.01]), "a repeated frequency"),
        (dict(frequencies=np.linspace(0.01, 0.1, 65)), "65 frequencies"),
        (dict(frequencies=[0.01, 6.01 / (2.0 * np.pi)]), "pi f de > 6"),
        (dict(max_shift=-1.0), "max_shift < 0"),
        (dict(max_shift=None), "max_shift None"),
        (dict(max_shift=np.nan), "max_shift NaN"),
        (dict(max_shift="far"), "max_shift not a number"),
        (dict(max_shift=True), "max_shift a bool"),
        (dict(max_shift=14.0), "7 cells, more than h - min_samples = 6"),
        (dict(max_shift=12.0, min_samples=5), "6 cells, more than h - min_samples = 5"),
        (dict(max_shift=2.0 * 65, half_length=400.0), "65 cells, more than 64"),
        (dict(cells=[40 * 50]), "a cell outside the grid"),
        (dict(cells=[0.5]), "a cell that is no integer"),
        (dict(angle=np.nan), "angle NaN"),
        (dict(angle=[0.1, 0.2, 0.3]), "three angles for two cells"),
        (dict(half_length=3.0), "h = 1"),
        (dict(half_length=2.0 * 1025), "h > 1024"),
        (dict(swath=-1.0), "swath < 0"),
        (dict(swath=2.0 * 33), "swath > 32 cells"),
        (dict(delta=-0.5), "delta < 0"),
        (dict(delta=np.inf), "delta inf"),
        (dict(min_samples=1), "min_samples < 2"),
        (dict(min_samples=11), "min_samples > h"),
        (dict(min_samples=4.5), "min_samples no integer"),
        (dict(data=np.zeros((40, 50))), "data no DEMGrid"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_channels(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device: the whole range of the shift, the largest the call takes, pi f de = 6 itself
    for kw in (dict(), dict(max_shift=13.9), dict(max_shift=2.0 * 64, half_length=400.0), dict(max_shift=0.0, return_shift=True),
               dict(frequencies=[6.0 / (2.0 * np.pi)]), dict(frequencies=0.02), dict(frequencies=np.geomspace(0.001, 0.9, 64)),
               dict(max_shift=4.0, swath=6.0, return_curve=True, return_shift=True, delta=0.0, min_samples=6)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_channels(**dict(ok, **kw))


def test_check_args_floors_to_cells():
    from scarplet_amd import channels
    a = channels.check_args((40, 50), 2.0, [3, 77], 0.1, 20.0, FS, 5.9, 5.9, 1.0, 4)
    assert (a.h, a.w, a.D, a.de, a.delta, a.min_samples) == (10, 2, 2, 2.0, 1.0, 4)
    assert a.frequencies.dtype == np.float64 and a.frequencies.flags.c_contiguous and np.array_equal(a.frequencies, FS)
    assert np.array_equal(a.cells, [3, 77]) and np.array_equal(a.sa, np.sin([0.1, 0.1])) and np.array_equal(a.ca, np.cos([0.1, 0.1]))
    assert channels.check_args((40, 50), 2.0, [3], 0.1, 20.0, FS, 0, 0, 1.0, 4).D == 0
    assert (_lib.CHANNEL_MAX_FREQS, channels.MAX_ARG) == (64, 6.0)


def test_matcher_route_validates():
    import scarplet_amd as sl

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    for kw in (dict(max_shift=-1.0), dict(max_shift=14.0), dict(frequencies=[0.02, 0.01]), dict(frequencies=[1.0]),
               dict(min_samples=11), dict(swath=-1.0)):
        with pytest.raises(ValueError):
            sl.Matcher.fit_channels(Held(), [3, 77], 20.0, **dict(dict(frequencies=FS, angle=0.1), **kw))
    Held.whole = False
    with pytest.raises(ValueError, match="fit_channels needs the whole DEM"):
        sl.Matcher.fit_channels(Held(), [3, 77], 20.0, FS, angle=0.1)


# ---- the table ------------------------------------------------------------------------------------------------------------
FIELDS = ("row", "col", "cell", "n", "f_index", "lo_index", "hi_index", "status", "f", "f_lo", "f_hi", "a", "b", "c0", "sse", "rmse",
          "shift_index", "shift", "depth", "sigma", "width", "width_lo", "width_hi", "area", "curvature", "centre_row", "centre_col")


def test_the_table_has_the_fields_of_the_docs():
    from scarplet_amd import channels
    assert channels.FIT_DTYPE.names == FIELDS
    rows = np.zeros(3, dtype=_lib.PROFILE_SHIFT_DTYPE)
    rows["cell"], rows["a"], rows["kt"], rows["kt_lo"], rows["kt_hi"] = [7, 53, 104], [-0.5, 1.0, np.nan], [0.05, 0.1, np.nan], \
        [0.04, 0.1, np.nan], [0.05, 0.2, np.nan]
    rows["kt_index"], rows["status"], rows["shift_index"], rows["shift"] = [3, 1, -1], [0, 8, 33], [2, -3, 0], [4.0, -6.0, np.nan]
    sa, ca = np.sin([0.0, 0.3, 0.3]), np.cos([0.0, 0.3, 0.3])
    t = channels._table(rows, 50, sa, ca, label=[3, 3, 4])
    assert t.dtype.names == FIELDS + ("label",) and t.dtype["label"] == np.int32
    assert list(t["row"]) == [0, 1, 2] and list(t["col"]) == [7, 3, 4] and list(t["f_index"]) == [3, 1, -1]
    assert list(t["f"][:2]) == [0.05, 0.1] and list(t["shift_index"]) == [2, -3, 0] and list(t["status"]) == [0, 8, 33]
    want = cr.derived(rows["kt"][:2], rows["kt_lo"][:2], rows["kt_hi"][:2], rows["a"][:2])
    for f, v in want.items():
        assert np.allclose(t[f][:2], v, rtol=1e-15, atol=0), f
    assert list(t["depth"][:2]) == [0.5, -1.0]                             # a channel, a ridge
    assert np.all(t["width_lo"][:2] <= t["width"][:2]) and np.all(t["width"][:2] <= t["width_hi"][:2])
    # width is the full width at half depth: exp(-(pi f width / 2)^2) = 1 / 2; sigma the Gaussian's; area its integral
    assert np.allclose(np.exp(-(np.pi * t["f"][:2] * t["width"][:2] / 2) ** 2), 0.5, rtol=1e-15)
    assert np.allclose(np.exp(-(np.pi * t["f"][:2] * t["sigma"][:2]) ** 2), np.exp(-0.5), rtol=1e-15)
    s = np.linspace(-400.0, 400.0, 800001)
    assert abs(np.sum(0.5 * np.exp(-(np.pi * 0.05 * s) ** 2)) * (s[1] - s[0]) - t["area"][0]) <= 1e-9
    assert t["centre_row"][0] == 0.0 and t["centre_col"][0] == 9.0
    assert t["centre_row"][1] == 1 + 3 * np.sin(0.3) and t["centre_col"][1] == 3 - 3 * np.cos(0.3)
    assert all(np.isnan(t[f][2]) for f in cr.DERIVED + ("f", "f_lo", "f_hi", "a"))     # (a row that is not fitted)


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_the_wrapper_fits_its_signature():
    """Context.channel_profiles through a library that records its calls, on the context's DEM and on z, each optional
    output on and off: every recorded call fits its SIGNATURES entry argument for argument (tests/test_fit_binding_host.py)."""
    K, F = 3, 2
    cells, sa, ca = np.array([5, 7, 9], dtype=np.int64), np.array([0.0, 0.6, 0.8]), np.array([1.0, 0.8, 0.6])
    freqs, z = np.array([0.05, 0.1]), np.arange(20.0).reshape(4, 5)
    ctx = fake_context()
    seen = set()
    for zz, curve, plane in itertools.product((None, z), (False, True), (False, True)):
        got = ctx.channel_profiles(cells, sa, ca, freqs, 4, 1, 2, 1.5, 1.0, 2, curve=curve, shift_plane=plane, z=zz)
        name, h, args = ctx.lib.log[-1]
        assert name == "sc_channel_profiles" + ("_dem" if zz is not None else "")
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
        assert own[3] == K and own[5] == F and own[6:12] == (4, 1, 2, 1.5, 1.0, 2)      # K; F; h, w, D, de, delta, min_samples
        assert C.cast(own[4], C.c_void_p).value == freqs.ctypes.data
        rows, sse, shifts = got
        assert rows.shape == (K,) and rows.dtype == _lib.PROFILE_SHIFT_DTYPE
        assert (sse is None) == (not curve) and (shifts is None) == (not plane)
        assert sse is None or (sse.shape == (K, F) and sse.dtype == np.float64 and sse.flags.c_contiguous)
        assert shifts is None or (shifts.shape == (K, F) and shifts.dtype == np.int8 and shifts.flags.c_contiguous)
    assert seen == {"sc_channel_profiles", "sc_channel_profiles_dem"}
    # the list is sc_fit_profiles_shift's
    for twin in ("", "_dem"):
        assert _lib.SIGNATURES["sc_channel_profiles" + twin] == _lib.SIGNATURES["sc_fit_profiles_shift" + twin]
    # ... and the names stay out of the fit family's count
    assert not [n for n in _lib.SIGNATURES if "channel" in n and n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_header_constants_and_abi(tmp_path):
    prog = tmp_path / "channel.c"
    prog.write_text('#include <stdio.h>\n#include "scarplet_hip.h"\nint main(void) {\n'
                    '  printf("%d %g %d %d %d %zu\\n", SC_CHANNEL_MAX_FREQS, SC_CHANNEL_MAX_ARG, SC_PROFILE_MAX_SHIFT, SC_K_COUNT, '
                    'SC_ABI_VERSION, sizeof(sc_profile_shift_fit));\n  return 0;\n}\n')
    exe = tmp_path / "channel"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    from scarplet_amd import channels
    assert subprocess.check_output([str(exe)]).split() == [b"%d" % _lib.CHANNEL_MAX_FREQS, b"%g" % channels.MAX_ARG,
                                                           b"%d" % _lib.PROFILE_MAX_SHIFT, b"%d" % len(_lib.K_NAMES), b"10",
                                                           b"%d" % _lib.PROFILE_SHIFT_DTYPE.itemsize]
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in ("sc_channel_profiles", "sc_channel_profiles_dem"):
        assert re.search(r"\bint %s\s*\(" % n, code), n
    assert '"channel_terms"' in txt


def test_library_exports_the_channel_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("sc_channel_profiles", "sc_channel_profiles_dem"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    a, b = _lib.SIGNATURES["sc_channel_profiles"][1], _lib.SIGNATURES["sc_channel_profiles_dem"][1]
    assert len(a) == 16 and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bsc_channel\.hip\b", src, flags=re.M)


def test_channel_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_channel.hip")
    for k in ("k_ch_fit<true>", "k_ch_fit<false>"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD
    assert t["k_ch_table"]["scratch"] == 0 and t["k_ch_terms"]["scratch"] == 0


# ---- the synthetic surface ------------------------------------------------------------------------------------------------
def test_synthetic_channel_is_synthetic_scarp_with_a_trough():
    from scarplet_amd import synthetic
    a = synthetic.synthetic_channel(64, ny=48, f0=0.05, depth=2.0, sigma=0.05, theta=0.3)
    b = synthetic.synthetic_scarp(64, ny=48, sigma=0.05, theta=0.3)
    za, zb = np.asarray(a._griddata), np.asarray(b._griddata)
    assert za.shape == zb.shape == (48, 64) and a._georef_info.dx == b._georef_info.dx == 1.0
    # the same noise draw and the same line: without noise the difference is the two shapes' (float32 storage on both sides)
    a0 = np.asarray(synthetic.synthetic_channel(64, ny=48, f0=0.05, depth=2.0, sigma=0.0, theta=0.3)._griddata, dtype=np.float64)
    b0 = np.asarray(synthetic.synthetic_scarp(64, ny=48, sigma=0.0, theta=0.3)._griddata, dtype=np.float64)
    assert np.abs((za - a0) - (zb - b0)).max() <= 1e-6
    x, y = np.linspace(-32, 32, 64), np.linspace(-24, 24, 48)
    yrot = -x[None, :] * np.cos(0.3) + y[:, None] * np.sin(0.3)
    assert np.abs(a0 - (-2.0 * np.exp(-(np.pi * 0.05 * yrot) ** 2) + 0.01 * yrot)).max() <= 1e-6
    assert np.asarray(synthetic.synthetic_channel(32, dtype=np.float64)._griddata).min() < -0.8


# ---- the restatements -----------------------------------------------------------------------------------------------------
def test_the_case_list():
    cases = cr.gpu_cases()
    assert [c["name"] for c in cases] == cr.NAMES
    by = {c["name"]: c for c in cases}
    for c in cases:
        assert 0 <= c["D"] <= min(_lib.PROFILE_MAX_SHIFT, c["h"] - c["min_samples"]) and len(c["cells"]) <= 300
        f = c["frequencies"]
        assert 1 <= len(f) <= 64 and np.all(np.diff(f) > 0) and (np.pi * f[-1]) * c["de"] <= 6.0
        big = {cr.NAMES[0]: (600, 600), "F = 64, h = 100, D = 8": (256, 256)}
        assert c["z"].shape == big.get(c["name"], (96, 128))
    c = by[cr.NAMES[0]]
    assert (c["h"], c["w"], c["D"], len(c["frequencies"]), len(c["cells"])) == (100, 2, 8, 28, 100)
    c = by["de = 2, h30 w5 D4 F12"]
    assert (c["de"], c["h"], c["w"], c["D"], len(c["frequencies"])) == (2.0, 30, 5, 4, 12)
    c = by["D = h - min_samples"]
    assert (c["h"], c["D"]) == (12, 8) and c["D"] == c["h"] - c["min_samples"]
    assert by["D = 0"]["D"] == 0
    c = by["one frequency"]
    assert len(c["frequencies"]) == 1 and c["D"] == 3
    c = by["F = 35, D = 8"]
    P = len(c["frequencies"]) * (2 * c["D"] + 1)
    assert P == 595 and P % 64 and 64 % 35                              # a partial last round; a frequency's pairs in several
    assert 8 * (2 * (c["h"] + c["D"]) + 1) * 35 <= 65536                 # the table in LDS
    c = by["F = 64, h = 100, D = 8"]
    assert len(c["frequencies"]) * (2 * c["D"] + 1) == 1088 and 8 * (2 * (c["h"] + c["D"]) + 1) * 64 == 111104   # ... in global memory
    assert len(by["borders and corners"]["cells"]) % 4 and len(by["K = 1"]["cells"]) == 1 and len(by["no cell"]["cells"]) == 0
    assert by["repeated cells"]["delta"] == 0.0


def test_the_border_and_nan_cases_have_the_cells_they_are_about():
    by = {c["name"]: c for c in cr.gpu_cases()}
    c = by["borders and corners"]
    rows = cr.restate(c)
    n, st = np.array([r["n"] for r in rows]), np.array([r["status"] for r in rows])
    full = n == 2 * c["h"] + 1
    assert (st == 1).sum() >= 4 and ((st & 1 == 0) & ~full).sum() >= 4 and full.sum() >= 15
    groups = [full[k:k + 4] for k in range(0, len(full), 4)]
    assert sum(g.any() and not g.all() for g in groups) >= 8             # complete and clipped profiles share a workgroup
    c = by["NaN cells"]
    rows = cr.restate(c)
    n, st = np.array([r["n"] for r in rows]), np.array([r["status"] for r in rows])
    assert list(n[-3:]) == [39, 39, 20] and list(st[-3:] & 1) == [0, 0, 1]   # the centre, j = 1 and 2, a whole side
    assert ((st & 1 == 0) & (n < 41)).sum() >= 8 and (n == 41).sum() >= 8    # both routes in one launch
    rows = cr.restate(by["no live pair"])
    assert [r["status"] for r in rows] == [33, 6, 6] and rows[0]["n"] == 33 and np.isnan(rows[0]["curve"]).all()
    assert all(r["dof"] == r["n"] - 3 for r in cr.restate(by["D = 0"])) and not any(r["status"] & 8 for r in cr.restate(by["D = 0"]))


@pytest.mark.parametrize("name", cr.NAMES)
def test_the_two_restatements_agree(name):
    """Float64 lstsq on equilibrated columns against longdouble Gram-Schmidt, on every input of the GPU tests: RTOL / 100 in
    every sse and every coefficient (relative to the profile's range), every live pair under the condition cap, the same
    pairs dead, and no d_i, no index and no status decided differently.  Measured over all cases: 1.1e-15 in the sse,
    3.4e-14 in the coefficients, a largest condition number of 10 (h = 12 with D = 8); no frequency grid had to be cut."""
    case = {c["name"]: c for c in cr.gpu_cases()}[name]
    a, b = cr.case_pairs(case), cr.case_pairs(case, longdouble=True)
    worst = {"sse": 0.0, "coef": 0.0, "cond": 0.0, "usable": 0, "dead": 0}
    scale = np.array([1.0, case["h"] * case["de"], 1.0])
    for x, y in zip(a, b):
        assert x["n"] == y["n"] and x["usable"] == y["usable"]
        if not x["usable"]:
            continue
        worst["usable"] += 1
        assert x["cond"] <= cr.COND_MAX, (x["cell"], x["cond"])
        gy = y["grid"].astype(np.float64)
        live = ~np.isnan(gy)
        assert np.array_equal(np.isnan(x["grid"]), ~live), x["cell"]
        worst["dead"] += int((~live).sum())
        if live.any():
            worst["sse"] = max(worst["sse"], float(np.max(np.abs(x["grid"][live] - gy[live]) / gy[live])))
            worst["coef"] = max(worst["coef"], float(np.max(np.abs(x["coefs"][live] - y["coefs"][live].astype(np.float64)) * scale))
                                / x["ptp"])
        worst["cond"] = max(worst["cond"], x["cond"])
    print("%s: %s" % (name, worst))
    assert worst["sse"] <= cr.RTOL / 100 and worst["coef"] <= cr.RTOL / 100, worst
    for x, y in zip(cr.restate(case), cr.restate(case, longdouble=True)):
        for f in ("n", "dof", "f_index", "lo_index", "hi_index", "status", "shift_index"):
            assert x[f] == y[f], (name, x["cell"], f, x[f], y[f])
        assert np.array_equal(x["shifts"], y["shifts"]), (name, x["cell"])


def test_the_condition_number_stays_low_over_the_widths_a_profile_resolves():
    """docs/channels.md: the tolerances of the family stand on a column-scaled design matrix of condition number <= 1e3.  The
    Gaussian's (1, s, column) must keep an order of magnitude under that cap for widths between half a cell and h / 2 cells at
    every shift, also on a profile clipped four points past the centre, where a shifted trough's centre leaves the profile.
    Measured: 77 at worst (the widest trough on the clipped profile, shifted off it); 2.7 on the recovery surface."""
    h, D = 100, 8
    f = cr.freqs_of_sigma(np.geomspace(0.5, h / 2, 24))
    worst = 0.0
    for j in (np.arange(-h, h + 1), np.arange(-h, 5), np.arange(-4, h + 1)):
        s = j.astype(np.float64)
        cols = np.array([cr.gauss_column(j, d, 1.0, fi) for fi in f for d in range(-D, D + 1)])
        worst = max(worst, float(cr.conds(s, cols).max()))
    print("largest condition number: %.1f" % worst)
    assert worst <= cr.COND_MAX / 10


# ---- what it does: the recovery surface of docs/channels.md ---------------------------------------------------------------------
def recovery_rows(noise, D):
    R = cr.REC
    z, cells, theta, off = cr.recovery_case(noise)
    if noise == R["noise"] and D == R["D"]:
        return cr.restate(cr.gpu_cases()[0]), off, theta
    return cr.fit_channels(z, 1.0, cells, theta, R["h"], R["w"], D, R["frequencies"]), off, theta


def test_the_shift_finds_the_width_the_fixed_centre_misses():
    """600 x 600, theta = 0.2, a trough 6.55 cells wide (sigma) and 1 deep, noise 0.05, 100 cells up to six columns off its
    line, h = 100, w = 2, 28 frequencies in 12 % steps.  Measured: the true frequency in 100 of 100 cells with D = 8 (depths
    0.984 to 1.010, every interval one frequency wide), in 33 of 100 with D = 0 (median depth 0.899, 0.666 at worst)."""
    R = cr.REC
    with_shift, off, theta = recovery_rows(R["noise"], R["D"])
    without, _, _ = recovery_rows(R["noise"], 0)
    hit = sum(r["f_index"] == R["index"] for r in with_shift)
    miss = sum(r["f_index"] == R["index"] for r in without)
    depth = np.array([-r["a"] for r in with_shift])
    print("true frequency: %d of 100 at D = 8 (depth %.3f .. %.3f), %d of 100 at D = 0 (median depth %.3f, least %.3f)"
          % (hit, depth.min(), depth.max(), miss, np.median([-r["a"] for r in without]), min(-r["a"] for r in without)))
    assert len(with_shift) == 100 and hit >= 95
    assert miss <= 50
    assert (hit, miss) == (100, 33)                                        # the counts docs/channels.md quotes
    assert all(r["dof"] == r["n"] - 4 for r in with_shift) and all(r["dof"] == r["n"] - 3 for r in without)
    assert max(r["cond"] for r in with_shift) <= 3.0


def test_without_noise_the_shift_is_the_offset_along_the_profile():
    R = cr.REC
    rows, off, theta = recovery_rows(0.0, R["D"])
    dev = np.abs(np.array([r["shift_index"] for r in rows]) + off * np.cos(theta))
    print("|shift + offset cos(theta)| <= %.3f cells" % dev.max())
    assert dev.max() <= 1.2 and not any(r["status"] & 8 for r in rows)
    assert all(r["f_index"] == R["index"] for r in rows)


def test_the_search_and_the_fit_agree_on_sign_and_scale():
    """docs/channels.md, "Against the search": the oracle's Channel search at the trough's own frequency over orientations
    within 0.3 rad, and the restatement's fit at the 312 cells of the line that lie 100 cells and more from every border, with
    the search's own angle.  Measured: amp > 0 and a < 0 in every cell, and a median amp / curvature of 0.9856 (0.947 to
    1.026).  tests/test_gpu_channels.py holds the device to these two figures."""
    import scarplet_oracle as so
    S = cr.SEARCH
    z = cr.channel_z(S["n"])
    res = so.best_fit_one_age(z, 1.0, 1.0, so.RICKER, S["scale"], S["f0"], ang_max=S["ang"], ang_min=-S["ang"])
    cells = cr.line_cells(S["n"], S["n"], np.arange(S["margin"], S["n"] - S["margin"]))
    amp, ang = res[0].ravel()[cells], res[2].ravel()[cells]
    rows = cr.fit_channels(z, 1.0, cells, ang, S["h"], S["w"], S["D"], cr.search_frequencies())
    a, f = np.array([r["a"] for r in rows]), np.array([r["f"] for r in rows])
    share = float(((amp > 0) & (a < 0)).mean())
    ratio = float(np.median(amp / cr.derived(f, f, f, a)["curvature"]))
    print("%d cells: amp > 0 and a < 0 in %.4f of them, median amp / curvature %.4f" % (len(cells), share, ratio))
    assert len(cells) == 312 and share == cr.SEARCH_SHARE and abs(ratio - cr.SEARCH_RATIO) <= 5e-5
