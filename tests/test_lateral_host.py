"""sl.lateral_offsets on the CPU: argument validation before the library is loaded, the table and the exports, the layout
of sc_lateral_fit and the header's ABI, the exported symbols, the kernel's register budget, and the numpy restatement
(tests/lateral_reference.py) on the planted strike-slip surface of docs/lateral.md."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lateral_reference as lr
from scarplet_amd import _lib, lateral

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("row", "col", "cell", "n", "lag", "lo", "hi", "status", "offset", "offset_lo", "offset_hi", "mse", "rho", "dz",
          "tilt")


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
    ok = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0, near=4.0, far=12.0, max_offset=8.0)   # h 10, q 2..6, D 4
    bad = [
        (dict(near=1.9), "near below the cell size"),
        (dict(near=0.0), "near 0"),
        (dict(near=np.nan), "near NaN"),
        (dict(far=3.9), "far below near"),
        (dict(far=np.inf), "far inf"),
        (dict(far="wide"), "far not a number"),
        (dict(max_offset=-0.1), "max_offset < 0"),
        (dict(max_offset=np.nan), "max_offset NaN"),
        (dict(max_offset=True), "max_offset a bool"),
        (dict(min_samples=2), "min_samples < 3"),
        (dict(min_samples=22), "min_samples > 2 h + 1"),
        (dict(min_samples=8.0), "min_samples not an integer"),
        (dict(min_samples=True), "min_samples a bool"),
        (dict(half_length=1.9), "h < 1"),
        (dict(half_length=-1.0), "half_length < 0"),
        (dict(half_length=2.0 * 1025), "h above SC_PROFILE_MAX_HALF"),
        (dict(far=2.0 * 1025, near=2.0 * 1000), "q1 above SC_LATERAL_MAX_FAR"),
        (dict(far=2.0 * 66), "a band of 65 lines"),
        (dict(max_offset=2.0 * 256), "D above SC_LATERAL_MAX_LAG"),
        (dict(delta=-1.0), "delta < 0"),
        (dict(delta=np.nan), "delta NaN"),
        (dict(angle=[0.1, np.nan]), "angle NaN"),
        (dict(angle=np.nan), "a NaN angle for all"),
        (dict(angle=[0.1, 0.2, 0.3]), "angles of another length"),
        (dict(cells=[3, 2000]), "a cell off the grid"),
        (dict(cells=[-1]), "a negative cell"),
        (dict(cells=([3], [50])), "a column off the grid"),
        (dict(cells=[0.5, 1.5]), "cells not integers"),
        (dict(data=np.zeros((40, 50))), "data not a DEMGrid"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.lateral_offsets(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device
    for kw in (dict(), dict(near=2.0, far=2.0), dict(max_offset=0), dict(min_samples=3), dict(min_samples=21),
               dict(far=2.0 * 65), dict(max_offset=2.0 * 255), dict(return_curve=True, delta=0.0), dict(cells=[])):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.lateral_offsets(**dict(ok, **kw))


def test_check_args_counts_cells():
    idx, sa, ca, h, q0, q1, D, de, d, ms = lateral.check_args((40, 50), 2.0, [3, 77], 0.1, 21.9, 4.0, 13.9, 9.9, 1.0, 8)
    assert (h, q0, q1, D, de, d, ms) == (10, 2, 6, 4, 2.0, 1.0, 8)
    assert idx.tolist() == [3, 77] and np.array_equal(sa, np.sin([0.1, 0.1])) and np.array_equal(ca, np.cos([0.1, 0.1]))


def test_matcher_route_validates():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(near=1.0), dict(far=3.0), dict(max_offset=-1.0), dict(min_samples=2), dict(strike="both")):
        args = dict(half_length=20.0, near=4.0, far=12.0, max_offset=8.0)
        args.update(kw)
        with pytest.raises(ValueError):
            sl.Matcher.lateral_offsets(Held(), tr, **args)
    part = Held()
    part.whole = False
    with pytest.raises(ValueError):
        sl.Matcher.lateral_offsets(part, tr, 20.0, 4.0, 12.0, 8.0)
    wrong = traces.Traces(np.zeros((4, 5), dtype=bool), np.zeros((4, 5), dtype=np.int32),
                          traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    with pytest.raises(ValueError):
        sl.Matcher.lateral_offsets(Held(), wrong, 20.0, 4.0, 12.0, 8.0)


def test_table_fields_and_exports():
    assert lateral.FIT_DTYPE.names == FIELDS
    assert all(lateral.FIT_DTYPE.fields[f][0] == np.float64 for f in FIELDS[8:])
    assert all(lateral.FIT_DTYPE.fields[f][0] == np.int32 for f in FIELDS[3:8])
    assert tuple(f for f, _ in lr.FIELDS) == FIELDS
    import scarplet_amd as sl
    assert sl.lateral_offsets is lateral.lateral_offsets and hasattr(sl.Matcher, "lateral_offsets")
    t = lateral._table(np.zeros(2, dtype=_lib.LATERAL_FIT_DTYPE), 50, label=np.array([4, 9]))
    assert t.dtype.names == FIELDS + ("label",) and t["label"].tolist() == [4, 9]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_lateral_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_lateral_fit, _lib.LATERAL_FIT_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_lateral_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_lateral_fit, %s));\n' % f for f in names)
    prog = tmp_path / "lateral.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d %d %d\\n", SC_K_COUNT, SC_ABI_VERSION, SC_LATERAL_MAX_LAG, SC_LATERAL_MAX_BAND,'
                    ' SC_LATERAL_MAX_FAR);\n  return 0;\n}\n')
    exe = tmp_path / "lateral"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [11, 10, 255, 64, 1024]
    assert ctypes.sizeof(S) == 88 and dt.itemsize == 88 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert tuple(names) == FIELDS[2:]
    assert (_lib.LATERAL_MAX_LAG, _lib.LATERAL_MAX_BAND, _lib.LATERAL_MAX_FAR) == (255, 64, 1024)
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


LATERAL_CALLS = ("sc_lateral_offsets", "sc_lateral_offsets_dem")


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in LATERAL_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert len(_lib.SIGNATURES[n][1]) == 14 + (3 if n.endswith("_dem") else 0)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in LATERAL_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_lateral.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)


def test_lateral_kernel_fits_its_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_lateral.hip")
    assert "k_lt_fit" in t, sorted(t)
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)                        # four waves per SIMD


# ---- the restatement on the planted surface --------------------------------------------------------------------------------
def _planted(theta, angle=None, s=lr.PLANT_S):
    z = lr.planted_surface(theta, s=s)
    return lr.lateral_offsets(z, 1.0, lr.planted_stations(theta), theta if angle is None else angle, **lr.PLANT)[0]


@pytest.mark.parametrize("theta", lr.PLANT_THETAS)
def test_restatement_finds_the_planted_offset(theta):
    """s = 7.3 cells, noise 0.02, h = 40, band 2..6, D = 20, eleven stations on the line: lag 7 at every station and
    |offset - 7.3| <= 0.1.  Measured with this restatement: lo = hi = 7 everywhere, |offset - 7.3| <= 0.022,
    rho >= 0.996 at the three strikes."""
    rows = _planted(theta)
    print(rows["lag"].tolist(), np.abs(rows["offset"] - 7.3).max(), rows["rho"].min())
    assert len(rows) == 11 and (rows["lag"] == 7).all()
    assert (np.abs(rows["offset"] - 7.3) <= 0.1).all()
    assert (rows["status"] == 0).all() and (rows["n"] == 81).all()
    # each side keeps its mean and its line: the step of 0.5 and the differential tilt of 0.003 come back as dz and tilt
    # (dz also holds 0.02 Q between the bands' centres 8 cells apart and what the tilt makes of the lag)
    assert np.allclose(rows["tilt"], 0.003, atol=2e-3) and np.allclose(rows["dz"], 0.5 + 0.02 * 8, atol=0.1)


def test_the_sign_does_not_depend_on_the_angles_branch():
    """The same surface, the angle turned by pi: the sides swap and so does the direction - the same lag, the same sign."""
    a = _planted(0.3)
    b = _planted(0.3, angle=0.3 + np.pi)
    assert (a["lag"] == 7).all() and (b["lag"] == 7).all()
    assert (np.abs(b["offset"] - 7.3) <= 0.1).all()


def test_positive_is_right_lateral():
    """Strike 0 on a north-up raster with row 0 at the top: the +q side is the right (east) half, the strike points down
    (south).  A ridge that crosses the fault and sits 7 rows lower on the right half than on the left was carried to the
    right as seen from the left half: right-lateral, and positive."""
    r = np.arange(120, dtype=np.float64)[:, None] * np.ones((1, 90))
    c = np.ones((120, 1)) * np.arange(90)[None, :]
    ridge = lambda r0: np.exp(-0.5 * ((r - r0) / 3.0) ** 2) + 0.3 * np.exp(-0.5 * ((r - r0 - 17.0) / 2.0) ** 2)
    z = np.where(c <= 45, ridge(50.0), ridge(57.0))
    rows = lr.lateral_offsets(z, 1.0, [60 * 90 + 45], 0.0, 30, 2, 6, 12)[0]
    assert rows["lag"][0] == 7 and abs(rows["offset"][0] - 7.0) <= 0.1
    # the mirrored plant is left-lateral and negative
    assert (_planted(-1.1, s=-lr.PLANT_S)["lag"] == -7).all()


def test_a_constant_dem_ties_every_lag():
    """Nothing to correlate: every lag has mse 0, the first candidate - lag 0 - wins the tie, the interval is the whole
    range and rho has no value."""
    for z, angle in ((np.zeros((96, 80)), 0.3), (np.full((96, 80), 3.0), 0.0)):
        cells = np.array([40 * 80 + 40, 50 * 80 + 30, 48 * 80 + 41])
        rows, mse, _ = lr.lateral_offsets(z, 1.0, cells, angle, 10, 2, 6, 5)
        assert (mse == 0.0).all()
        assert (rows["lag"] == 0).all() and (rows["mse"] == 0.0).all() and np.isnan(rows["rho"]).all()
        assert (rows["lo"] == -5).all() and (rows["hi"] == 5).all() and (rows["status"] == 6).all()
        assert (rows["offset"] == 0.0).all() and (rows["dz"] == 0.0).all() and (rows["n"] == 21).all()


def test_a_station_without_a_lag():
    z = lr.rough_dem((96, 80), 1)
    rows, mse, _ = lr.lateral_offsets(z, 1.0, [0], 0.3, 5, 2, 9, 4, min_samples=11)
    assert rows["status"][0] == 1 and rows["n"][0] == 0 and rows["lag"][0] == 0 and rows["lo"][0] == 0 and rows["hi"][0] == 0
    assert all(np.isnan(rows[f][0]) for f in lr.FLOAT_FIELDS) and np.isnan(mse).all()
