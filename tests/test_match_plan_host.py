"""The search's launch plan (scarplet_amd/csrc/sc_match_plan.h) and the launch shapes of the inverse passes
(sc_fft_route.h) on the host.  tests/match_plan_check.cpp plans a few hundred seeded random descriptor lists - both
methods, maps, mixed kinds, equal and unequal run lengths, repeated orientations, masked templates, up to three times
SC_MAX_BATCH templates, a spread of cores and tile plans - and prints them: every field is held against the restatement of
tests/match_plan_reference.py.  Run without arguments it asserts the plan's properties on the same lists and on a sweep
of regular searches, and follows every planned chunk through the launch shapes of every route.  A program of its own
under AddressSanitizer and UBSan; nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

import match_plan_reference as mp

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "scarplet_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ builds this test's program: it is not on PATH"
    out = str(tmp_path_factory.mktemp("match_plan") / "match_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "match_plan_check.cpp"), "-o", out], check=True)
    return out


def test_the_plans_of_random_lists_are_the_restatement_s(exe):
    r = subprocess.run([exe, "print"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = mp.parse(r.stdout)
    assert len(cases) >= 300
    seen = dict(direct=0, fft=0, maps=0, batched=0, batch_sliced=0, long_run=0, masked=0, mixed_parity=0, repeated=0, no_slots=0,
                slots=0, over_a_batch=0, tail_rides=0, tail_halved=0, unequal=0)
    for k, (inp, templ, got) in enumerate(cases):
        want = mp.plan(inp, templ)
        for name in want:
            assert got[name] == want[name], (k, name, inp)
        seen["direct" if inp.method == mp.DIRECT else "fft"] += 1
        seen["maps"] += inp.to_maps
        nbs = [c.nb for c in got["chunks"]]
        seen["batched"] += max(nbs) > 1
        seen["batch_sliced"] += any(c.nb * c.n > mp.MAX_GROUP for c in got["chunks"]) and inp.method == mp.FFT
        seen["long_run"] += len({q.n for q in got["runs"]}) == 1 and got["runs"][0].n == mp.MAX_GROUP and len(got["runs"]) > 1
        seen["masked"] += any(t.masked for t in templ)
        seen["mixed_parity"] += len({mp.parity_of(t, inp) for t in templ}) > 1
        keys = [(templ[q.first].cc, templ[q.first].sc2) for q in got["runs"]]
        seen["repeated"] += len(set(keys)) < len(keys)
        seen["no_slots"] += inp.method == mp.FFT and inp.spectra and not inp.to_maps and got["n_slots"] == 0
        seen["slots"] += got["n_slots"] > 1
        seen["over_a_batch"] += len(templ) > mp.MAX_BATCH
        seen["unequal"] += len({q.n for q in got["runs"]}) > 2
        # the tail rule acted: a batch above what fills the chip, or two uneven ones where one would not do
        if inp.method == mp.FFT and max(nbs) > 1:
            w = [mp.want_fft(inp, c.n) for c in got["chunks"]]
            seen["tail_rides"] += any(c.nb > wc > 1 for c, wc in zip(got["chunks"], w))
            seen["tail_halved"] += any(1 < c.nb < wc and d.nb in (c.nb, c.nb - 1) and d.n == c.n and c.nb + d.nb > wc + wc // 4
                                       for c, d, wc in zip(got["chunks"], got["chunks"][1:], w))
    # the lists held what they were meant to hold
    assert all(v >= 5 for v in seen.values()), seen


def test_properties_of_the_plan_and_of_the_launch_shapes(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"match_plan: (\d+) checks, 0 failed; (\d+) row-pass launches, (\d+) refused", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > 10 ** 6 and int(m.group(2)) > 10 ** 5
    # no chunk the plan produces comes to fft_inverse_fold's "row pass: ... shares" refusal, on any route
    assert int(m.group(3)) == 0


def test_the_tile_plan_refusals(exe):
    r = subprocess.run([exe, "refusals"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split("\n")[:6] == ["ok", "bad tile plan", "circular axis needs T == n and the whole DEM",
                                        "circular axis needs T == n and the whole DEM", "tiles do not cover the core", "ok"]


def test_the_plan_is_decided_in_one_place():
    """match_impl and fft_inverse_fold ask the headers: neither decides a run, a batch, an offset, a slot, a slice or a share
    itself."""
    api = open(os.path.join(CSRC, "sc_api.hip")).read()
    body = api[api.index("\nstatic int match_impl("):api.index('extern "C" int sc_match_async(')]
    assert "sc_match_plan(" in body and "sc_match_plan_check(" in body
    for word in ("avail", "want", "hard", "look", "slot_of[r", "n_slots++", "off +=", "& ~", "nb = ", "SC_MAX_BATCH", "SC_MAX_ORIENT"):
        assert word not in body, word
    assert len(re.findall(r"launch_curv_alpha(_batch)?\(", api[api.index("// the hot path"):])) == 2      # one helper, both forms
    fft = open(os.path.join(CSRC, "sc_fft.hip")).read()
    body = fft[fft.index("\nint fft_inverse_fold("):]
    for call in ("fft_route_col_pairs(", "fft_route_nsplit_max(", "fft_route_row_slice(", "fft_route_nsplit(", "fft_route_nsplit_refused("):
        assert call in body, call
    for word in ("cap_t", "nsl", "lds_c", "split_waves", "c.split_max", "/ 4", "255", "SC_MAX_GROUP - 1"):
        assert word not in body, word
