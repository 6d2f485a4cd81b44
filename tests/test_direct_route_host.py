"""The real-space path's route (scarplet_amd/csrc/sc_direct_route.h) on the host: tests/direct_route_check.cpp sweeps core
extents, window boxes, long_runs and the variants 0 / 11 / 16 / 19 and asserts invariants - the slab a launch asks for
exists and holds its patch, the W4 class stages every template in one slab, the 512 patch is chosen only where its slab
fits.  Given the case table of tests/direct_classes.py it answers, with the route's own functions, which class, batch and
slab count every launch of every case takes: each case must reach what its name claims, and the table all eight
instantiations of k_direct2, both batch regimes, single- and multi-slab staging and the narrow-DEM wrap path.
A program of its own under AddressSanitizer and UBSan; nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import direct_classes as dc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "scarplet_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ builds this test's program: it is not on PATH"
    out = str(tmp_path_factory.mktemp("direct_route") / "direct_route_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "direct_route_check.cpp"), "-o", out], check=True)
    return out


def ask(exe, lines):
    r = subprocess.run([exe, "cases"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def reached(exe, c):
    """What the launches of a case take, by the route's own functions: (classes, batched, slabs, narrow, launches)."""
    ny, nx, _ = dc.DEMS[c["dem"]]
    want = int(ask(exe, ["R 0 %d %d 1 1 0 0 1 1" % (ny, nx)])[0][7])
    long_of_run = None
    if "make" not in c:
        ans = ask(exe, dc.long_run_queries(c))
        long_of_run = np.zeros(len(c["angles"]), dtype=bool)
        for (_, ib, _, lr) in ans:
            long_of_run[int(ib)] |= lr == "1"
    lines, launches = dc.route_queries(c, long_of_run, want)
    ans = ask(exe, lines)
    classes, slabs, narrow, per_launch = set(), 1, set(), {}
    for (_, k, NB, RW, share, w4, lds, want_k, na, ns, nar) in ans:
        cls = (int(NB), int(RW), share == "1", w4 == "1")
        assert per_launch.setdefault(k, cls) == cls              # (one launch, one class)
        classes.add(cls)
        slabs = max(slabs, int(ns))
        narrow.add(nar == "1")
        assert int(want_k) == want
    assert len(narrow) == 1
    return classes, any(nb > 1 for (_, nb, _) in launches), slabs, narrow.pop(), launches


def test_route_invariants(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout, r.stdout


def test_variant_10_never_reaches_the_route(exe):
    """The box kernel (variant 10) has its own launcher: launch_direct leaves for it before it asks the route, and the
    host program refuses the question."""
    src = open(os.path.join(CSRC, "sc_kernels.hip")).read()
    body = src[src.index("\nint launch_direct("):]
    assert 0 < body.index("ctx->variant == 10") < body.index("return launch_direct_box(") < body.index("direct_route(")
    r = subprocess.run([exe, "cases"], input="R 0 100 100 9 9 1 10 9 9\n", capture_output=True, text=True)
    assert r.returncode == 2 and "variant 10" in r.stderr


def test_the_route_is_decided_in_one_place():
    """launch_direct and sc_match_plan (match_impl's planner) ask sc_direct_route.h: neither tests a patch size, a slab or
    the batch rule itself."""
    kern = open(os.path.join(CSRC, "sc_kernels.hip")).read()
    body = kern[kern.index("\nint launch_direct("):]
    assert "direct_route(" in body and "need256" not in body and "fits512" not in body and "wgs(" not in body
    api = open(os.path.join(CSRC, "sc_api.hip")).read() + open(os.path.join(CSRC, "sc_match_plan.h")).read()
    assert "direct_batch_want(" in api and "direct_long_runs(" in api
    assert "wg1" not in api and not re.search(r">=\s*16\.0", api)
    assert len(re.findall(r"#define\s+DR2_LDS_FLOATS", kern + api)) == 0


def test_share_min_is_the_table_s(exe):
    r = subprocess.run([exe, "share_min"], capture_output=True, text=True)
    assert r.returncode == 0 and int(r.stdout) == dc.SHARE_MIN


@pytest.mark.parametrize("name", [c["name"] for c in dc.CASES + dc.WINDOW_CASES])
def test_case_reaches_what_its_name_claims(exe, name):
    c = dc.CASE.get(name) or dc.WINDOW_CASE[name]
    classes, batched, slabs, narrow, launches = reached(exe, c)
    assert classes == c["classes"], (name, classes, launches)
    assert batched == c["batched"], (name, launches)
    assert (slabs > 1) == (c["slabs"] == "multi"), (name, slabs)
    assert narrow == c["narrow"], name
    # the name itself: "<NB,RW" or "W4", ",S" for the shared form, "multi-slab", "narrow"
    for (NB, RW, share, w4) in classes:
        tag = "W4" if w4 else "<%d,%d" % (NB, RW)
        assert tag in name and (("W4,S" if w4 else tag + ",S>") in name) == share, (name, (NB, RW, share, w4))
    assert ("multi-slab" in name) == (slabs > 1) and ("narrow" in name) == narrow, name


def test_table_covers_every_class_and_regime(exe):
    got = {}
    for c in dc.CASES + dc.WINDOW_CASES:
        classes, batched, slabs, narrow, _ = reached(exe, c)
        for cls in classes:
            got.setdefault(cls, set()).add((batched, slabs > 1, narrow))
    assert set(got) == dc.ALL_CLASSES, sorted(dc.ALL_CLASSES - set(got))
    every = set().union(*got.values())
    # both batch regimes for the 256 x 16 classes (the 256 x 8 class is always batched, the 512 x 16 never)
    for cls in (dc.C12S, dc.C12, dc.W4S, dc.W4):
        assert {b for (b, _, _) in got[cls]} == {True, False}, cls
    assert not any(b for cls in (dc.C22S, dc.C22) for (b, _, _) in got[cls])
    # several slabs at <1,1>, <1,2> and <2,2> (never W4), with and without the shared form where a case says so
    for cls in (dc.C11S, dc.C11, dc.C12S, dc.C22S, dc.C22):
        assert any(m for (_, m, _) in got[cls]), cls
    assert not any(m for cls in (dc.W4S, dc.W4) for (_, m, _) in got[cls])
    # the DEM narrower than its slab: at W4, <1,2> and <2,2>
    for cls in (dc.W4S, dc.W4, dc.C12S, dc.C22S):
        assert any(n for (_, _, n) in got[cls]), cls
    assert len(every) >= 4


def test_uploaded_windows_are_what_the_table_says():
    """The run-length window: every length from SHARE_MIN - 4 to SHARE_MIN + 8 at every start offset, as single runs and
    with one hole each; every transition between the row forms that the kernel's look-ahead meets."""
    rows = dc.run_length_rows()
    live = [r for r in rows if r != (0, 0)]
    assert sorted(live) == sorted((s, n) for n in range(dc.SHARE_MIN - 4, dc.SHARE_MIN + 9) for s in range(4))
    form = ["E" if r == (0, 0) else ("S" if r[1] >= dc.SHARE_MIN else "P") for r in rows]
    pairs = set(zip(form, form[1:]))
    assert {("S", "S"), ("S", "P"), ("P", "S"), ("P", "P"), ("S", "E"), ("E", "S")} <= pairs, pairs
    W = dc.run_length_window()
    n = len(rows)
    assert W.shape == (2 * n + 1, dc.RUNS_WIDTH) and not W[n].any()
    for k, (s, ln) in enumerate(rows):
        nz = np.flatnonzero(W[k])
        assert len(nz) == ln and (ln == 0 or (nz[0] % 4 == s and nz[-1] - nz[0] + 1 == ln)), k      # one run, no hole
        nz2 = np.flatnonzero(W[n + 1 + k])
        assert len(nz2) == max(ln - 1, 0) and (ln == 0 or (nz2[0] == nz[0] and nz2[-1] == nz[-1])), k   # one hole inside
    # the uploaded box keeps the start offsets: its first column is a multiple of four
    assert np.nonzero(W)[1].min() % 4 == 0
    # the parts (the W4 class) hold every row of the whole between them
    part_rows = sum(len(dc.run_length_window(k, 3, holes=(False,))) for k in range(3))
    assert part_rows >= len(rows) - 4 and part_rows <= len(rows)
    got = sorted(tuple(np.flatnonzero(r)[[0, -1]]) for k in range(3) for r in dc.run_length_window(k, 3, holes=(False,)) if r.any())
    assert got == sorted((8 + s, 8 + s + ln - 1) for (s, ln) in live)


def test_widest_window_dem_is_offered_the_512_patch_and_refused(exe):
    """tests/test_gpu_parity.py::test_direct_path_widest_window_on_a_large_dem: at 400 x 10300 the 512 x 16 patch gives 525
    workgroups - it is wanted - and a window of 2100 taps does not fit its slab: the launch takes <1,2,S>, whose slab holds two of
    the window's three rows at a time.
    (At 400 x 4600, that test's size before, the patch was never offered: 225 workgroups; a window of 2000 taps takes it.)"""
    def route(ch, cw, wh, ww):
        a = ask(exe, ["R 0 %d %d %d %d 1 0 %d %d" % (ch, cw, wh, ww, wh, ww)])[0]
        return (int(a[2]), int(a[3]), a[4] == "1", a[5] == "1"), int(a[9])
    assert route(400, 10300, 3, 2100) == (dc.C12S, 2)
    assert route(400, 10300, 3, 2000)[0] == dc.C22S
    assert route(400, 4600, 3, 2000)[0] == dc.C12S
