"""The segment-chunk rule of the fit drivers (scarplet_amd/csrc/sc_fit_chunk.h, option "fit_chunk") on the host:
tests/fit_chunk_check.cpp runs it over seeded random CSR arrays, and what it prints is held against the restatement of
tests/fit_chunk_reference.py and against the rule's properties, written out here without it.  A program of its own under
AddressSanitizer and UBSan; nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fit_chunk_reference as fc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ builds this test's program: it is not on PATH"
    out = str(tmp_path_factory.mktemp("fit_chunk") / "fit_chunk_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "fit_chunk_check.cpp"), "-o", out], check=True)
    return out


def csr(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


def random_cases():
    """(n, max_segs, max_cells, seg_start, aux_start or None, max_aux): seeded.  Sizes 0 come at the start, at the end and
    in runs; some segments are longer than the cell bound; bounds of 1 occur for every bound."""
    rng = np.random.default_rng(20261020)
    cases = []
    for i in range(400):
        S = int(rng.integers(1, 40))
        sizes = rng.choice([0, 0, 1, 2, 3, 7, 64, 65, 130, 2100], S)
        if i % 3 == 0:
            sizes[:int(rng.integers(1, 4))] = 0                          # empty segments first
        if i % 3 == 1:
            sizes[-int(rng.integers(1, 4)):] = 0                         # ... last
        if i % 4 == 0 and S > 6:
            k = int(rng.integers(1, S - 4))
            sizes[k:k + 3] = 0                                           # ... and in a run
        max_cells = int(rng.choice([1, 2, 64, 65, 100, 2100, 5000, 1 << 40]))
        max_segs = int(rng.choice([1, 2, 3, 5, 1 << 20]))
        n = int(rng.choice([0, 0, 1, 7, 64, 65, 100, 1 << 50]))
        aux, max_aux = None, 0
        if i % 2:
            aux = csr(rng.choice([0, 1, 1, 2, 5, 40], S))
            max_aux = int(rng.choice([1, 2, 6, 45, 1 << 21]))
        cases.append((n, max_segs, max_cells, csr(sizes), aux, max_aux))
    return cases


def run(exe, cases):
    text = []
    for n, max_segs, max_cells, seg, aux, max_aux in cases:
        text.append("%d %d %d %d %d %d" % (n, len(seg) - 1, max_segs, max_cells, aux is not None, max_aux))
        text.append(" ".join(map(str, seg)))
        if aux is not None:
            text.append(" ".join(map(str, aux)))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    return [[int(v) for v in line.split()] for line in lines]


def test_the_chunks_of_random_segments(exe):
    cases = random_cases()
    seen = dict(long_segment=0, segs_first=0, cells_first=0, aux_first=0, lowered=0, empty_first=0, empty_last=0, empty_run=0)
    for (n, max_segs, max_cells, seg, aux, max_aux), cuts in zip(cases, run(exe, cases)):
        S = len(seg) - 1
        cells = fc.bound(max_cells, n)
        assert cells == (max_cells if n <= 0 else min(max_cells, n))          # lowered, never raised
        assert cuts == fc.chunks(seg, max_segs, cells, aux, max_aux), (n, max_segs, max_cells, seg, aux, max_aux)
        # the chunks tile 0..S in order, each with at least one segment
        assert cuts[0] == 0 and cuts[-1] == S and all(b > a for a, b in zip(cuts, cuts[1:]))
        size = np.diff(seg)
        seen["empty_first"] += size[0] == 0
        seen["empty_last"] += size[-1] == 0
        seen["empty_run"] += bool(np.any((size[:-1] == 0) & (size[1:] == 0)))
        seen["lowered"] += cells < max_cells
        for s0, s1 in zip(cuts, cuts[1:]):
            over = [s1 - s0 > max_segs, seg[s1] - seg[s0] > cells, aux is not None and aux[s1] - aux[s0] > max_aux]
            # no chunk but one of a single segment exceeds a bound
            assert s1 - s0 == 1 or not any(over), (s0, s1, over)
            seen["long_segment"] += over[1]
            if s1 < S:
                # it could not have taken its successor's first segment
                more = [s1 + 1 - s0 > max_segs, seg[s1 + 1] - seg[s0] > cells,
                        aux is not None and aux[s1 + 1] - aux[s0] > max_aux]
                assert any(more), (s0, s1)
                seen["segs_first"] += more == [True, False, False]
                seen["cells_first"] += more == [False, True, False]
                seen["aux_first"] += more == [False, False, True]
    # the inputs held what they were meant to hold
    assert all(v >= 10 for v in seen.values()), seen


def test_bounds_of_one_and_the_default(exe):
    seg = csr([3, 0, 0, 5, 1, 0])
    big = 1 << 40
    cuts = run(exe, [(0, big, big, seg, None, 0), (1, big, big, seg, None, 0), (0, 1, big, seg, None, 0),
                     (0, big, big, seg, csr([1] * 6), 1), (5, big, 4, seg, None, 0), (-3, big, big, seg, None, 0)])
    assert cuts[0] == [0, 6]                                     # no bound reached: one chunk
    # a bound of one cell: every segment with cells goes alone, and the empty ones join a chunk that has room for them -
    # none after a segment above the bound
    assert cuts[1] == [0, 1, 3, 4, 6]
    assert cuts[2] == [0, 1, 2, 3, 4, 5, 6]                      # one segment a chunk
    assert cuts[3] == [0, 1, 2, 3, 4, 5, 6]                      # one item of the second array a chunk
    assert cuts[4] == cuts[1][:1] + [3, 4, 6]                    # the option does not raise the bound of 4 cells
    assert cuts[5] == [0, 6]                                     # (a negative n is refused by sc_set_option; here: no bound)
