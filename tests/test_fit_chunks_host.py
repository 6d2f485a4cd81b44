"""The segment-chunk rule of the fit drivers (scarplet_amd/csrc/sc_fit_chunk.h, option "fit_chunk") on the host:
tests/fit_chunk_check.cpp runs it over seeded random CSR arrays, and what it prints is held against the restatement of
tests/fit_chunk_reference.py and against the rule's properties, written out here without it.  So are the host arrays of
every chunk (its CSR arrays over cells and over blocks of 64, the segment of every cell, the interleaved directions) and
the cells a park holds, against the formulas of scarplet_amd/segments.py.  A program of its own under AddressSanitizer
and UBSan; nothing is loaded into Python."""
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


def stdin_of(cases):
    text = []
    for n, max_segs, max_cells, seg, aux, max_aux in cases:
        text.append("%d %d %d %d %d %d" % (n, len(seg) - 1, max_segs, max_cells, aux is not None, max_aux))
        text.append(" ".join(map(str, seg)))
        if aux is not None:
            text.append(" ".join(map(str, aux)))
    return "\n".join(text) + "\n"


def run(exe, cases):
    r = subprocess.run([exe], input=stdin_of(cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    return [[int(v) for v in line.split()] for line in lines]


def run_arrays(exe, cases):
    """Per case (cuts, totals, [per chunk a dict of G, start, blk, cseg, dir])."""
    r = subprocess.run([exe, "arrays"], input=stdin_of(cases), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = iter(r.stdout.strip().split("\n"))

    def named(name):
        head, _, rest = next(lines).partition(" ")
        assert head == name, (head, name)
        return np.array(rest.split(), dtype=np.int64)
    out = []
    for _ in cases:
        cuts = [int(v) for v in next(lines).split()]
        totals = named("totals")
        out.append((cuts, totals, [{k: named(k) for k in ("G", "start", "blk", "cseg", "dir")} for _ in cuts[1:]]))
    assert next(lines, None) is None
    return out


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


def test_the_host_arrays_of_every_chunk(exe):
    """What sc_sg_chunks sends up of a chunk, on the 400 cases: the numpy restatement, and the properties without it."""
    cases = random_cases()
    seen = dict(empty=0, one_block=0, a_rest=0, whole_blocks=0, no_cell=0)
    for (n, max_segs, max_cells, seg, aux, max_aux), (cuts, totals, chunks) in zip(cases, run_arrays(exe, cases)):
        seg = np.array(seg, dtype=np.int64)
        assert cuts == fc.chunks(seg, max_segs, fc.bound(max_cells, n), aux, max_aux)
        assert np.array_equal(totals, fc.block_totals(seg))
        assert totals[0] == 0 and np.array_equal(np.diff(totals), (np.diff(seg) + 63) // 64 + 1)
        for s0, s1, got in zip(cuts, cuts[1:], chunks):
            start, blk, cseg, G = fc.chunk_arrays(seg, s0, s1)
            assert np.array_equal(got["start"], start) and np.array_equal(got["blk"], blk)
            assert np.array_equal(got["cseg"], cseg) and got["G"].tolist() == [G]
            # the properties: the chunk's cells from 0, blk the CSR array of ceil(size / 64), G its last entry, cseg[k] the
            # segment whose range holds k, nothing from an empty segment, cell k0 + k at place k of the directions
            Sc, k0, m = s1 - s0, seg[s0], seg[s1] - seg[s0]
            size = np.diff(seg[s0:s1 + 1])
            assert len(got["start"]) == len(got["blk"]) == Sc + 1 and len(got["cseg"]) == m and len(got["dir"]) == 2 * m
            assert got["start"][0] == 0 and np.array_equal(np.diff(got["start"]), size)
            assert got["blk"][0] == 0 and np.array_equal(np.diff(got["blk"]), -(-size // 64)) and got["G"][0] == got["blk"][Sc]
            k = np.arange(m)
            assert np.all(got["start"][got["cseg"]] <= k) and np.all(k < got["start"][got["cseg"] + 1])
            assert not np.any(np.diff(got["blk"])[size == 0]) and not np.isin(got["cseg"], np.flatnonzero(size == 0)).any()
            assert np.array_equal(got["dir"][0::2], k0 + k) and np.array_equal(got["dir"][1::2], -(k0 + k + 1))
            seen["empty"] += bool(np.any(size == 0))
            seen["one_block"] += bool(np.any((size > 0) & (size < 64)))
            seen["whole_blocks"] += bool(np.any(size == 64))
            seen["a_rest"] += bool(np.any(size > 64))
            seen["no_cell"] += m == 0
    assert all(v >= 10 for v in seen.values()), seen


def test_the_park_cap_is_the_one_of_the_python_side(exe, monkeypatch):
    """sc_fit_park_cap in the four shapes of a park against scarplet_amd/segments.py (check_args, check_park,
    check_robust_park): a segment of `cap` cells passes there and one of cap + 1 is refused with both numbers in the
    message.  Under SC_SEGMENT_MAX_PARK, and under parks of 40 cells as tests/test_segment_ramp_host.py and
    tests/test_segment_robust_host.py set them."""
    from scarplet_amd import _lib, segments
    full = _lib.SEGMENT_MAX_PARK
    # (A, h, D or None, weight plane or None: no robust park, M or None, park)
    grid = [(A, h, D, wt, M, full) for A in (2, 35, 64) for h in (10, 66, 100)
            for D, wt, M in ((None, None, None), (0, None, None), (3, None, None), (None, None, 0), (None, None, 8), (None, None, 64),
                             (None, False, None), (None, True, None))]
    grid += [(2, 10, None, None, 6, 40 * 8 * (21 + 4 * 2 * 7)), (2, 10, None, None, None, 40 * 8 * (21 + 4 * 2 * 7)),
             (2, 10, None, False, None, 40 * 8 * (21 + 9 * 2)), (2, 10, None, True, None, 40 * 8 * (21 + 9 * 2)),
             (2, 10, 0, None, None, 40 * 8 * (21 + 9 * 2)), (5, 7, 3, None, None, 100000), (5, 7, None, None, None, 100000)]

    def shape(A, h, D, wt, M):
        """(prof, planes, columns, shift) as the drivers describe their park (sg_park, sc_fit.h)."""
        if wt is not None:
            return (2 * h + 1) * (2 if wt else 1), 9, A, 0
        return 2 * h + 1, 4, A * (M + 1 if M is not None else 1), int(D is not None)
    text = "".join("%d %d %d %d %d\n" % ((park,) + shape(A, h, D, wt, M)) for A, h, D, wt, M, park in grid)
    r = subprocess.run([exe, "cap"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    caps = [int(v) for v in r.stdout.split()]
    assert len(caps) == len(grid)
    named = {}
    for (A, h, D, wt, M, park), cap in zip(grid, caps):
        assert cap == fc.park_cap(park, *shape(A, h, D, wt, M))
        monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", park)
        named[A, h, D, wt, M, park == full] = cap
        msg = "a segment of %d cells: more than %d at" % (cap + 1, cap)

        def args(n):                                     # (what check_park and check_robust_park read of check_args' record)
            blank = segments.Args(*[None] * len(segments.Args._fields))
            return blank._replace(seg_start=np.array([0, 3, 3 + n]), ages=np.ones(A), h=h)
        if M is not None:
            segments.check_park(args(cap), M)
            with pytest.raises(ValueError, match=msg):
                segments.check_park(args(cap + 1), M)
        elif wt is not None:
            segments.check_robust_park(args(cap), wt)
            with pytest.raises(ValueError, match=msg):
                segments.check_robust_park(args(cap + 1), wt)
        elif park != full:
            # check_args itself, on cells of a 40 x 50 grid (repeated where the cap passes 2000)
            def call(n):
                return segments.check_args((40, 50), 2.0, np.arange(n) % 2000, np.ones(n, dtype=int), 0.1, 2.0 * h, 0,
                                           np.arange(1.0, A + 1.0), 1.0, 4, 1, shift=D is not None)
            assert np.array_equal(call(cap)[3], [0, cap])
            with pytest.raises(ValueError, match=msg):
                call(cap + 1)
    # the values that the host tests and the GPU tests of the families name
    assert named[2, 10, None, None, 6, False] == 40 and named[2, 10, None, False, None, False] == 40
    assert named[2, 10, None, True, None, False] == 26
    assert named[64, 66, None, None, 64, True] == 32008
    assert named[35, 100, None, False, None, True] == 1040447 and named[35, 100, None, True, None, True] == 748773
