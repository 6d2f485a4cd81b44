"""Traces on the MI355X at the layouts where labelling, scans, sort and reduction can go wrong (tests/trace_shapes.py,
pinned on the host by tests/test_trace_shapes_host.py): one component winding through every 32 x 32 tile, chains of
parents through many tile roots, thousands of merges on one root, a segment many radix and scan blocks long under a
single key, K == 1 (no sort pass) next to a large M, one giant among thousands of small segments, threshold and value
edges.  Every case is sl.extract_traces against the numpy reference through test_gpu_trace.check: thin, labels,
integer and peak fields equal, sums within 1e-12 of the summed absolute values.

Not reached: a fourth radix pass needs K > 2^24 segments, that is more than 6.7e7 cells and 2 GB of planes; the
first three passes are what the suite runs (test_gpu_trace's 4096 x 4096 planes give K > 65536)."""
import time

import numpy as np
import pytest

import scarplet_amd as sl
import trace_reference as tr
import trace_shapes as ts
from scarplet_amd import _lib, traces
from test_gpu_trace import SETTINGS, check, random_planes

pytestmark = pytest.mark.gpu

LO, HI, MC = ts.SETTINGS


@pytest.fixture(scope="module", autouse=True)
def warm_context():
    sl.extract_traces(np.ones((4, 8, 8)), 0.5)                         # (the context and its first launches)


def timed(planes, lo, hi, mc, what):
    """extract_traces with its K, largest segment and wall time (upload and read-back included) printed: the lines of
    profiles/trace_shapes.txt."""
    t0 = time.perf_counter()
    got = sl.extract_traces(planes, lo, hi, mc)
    wall = time.perf_counter() - t0
    n = got.segments["n_cells"]
    print("trace_shapes: %-40s %5d x %-5d K %6d  largest %7d  %8.2f ms"
          % (what, planes.shape[1], planes.shape[2], len(n), n.max() if len(n) else 0, 1e3 * wall))
    return got, wall


@pytest.mark.parametrize("name, variant", [(n, v) for n in ts.SMALL for v in ts.variants(n)])
def test_shape_against_reference(name, variant):
    mask, p = ts.planes(name, variant)
    got, _ = timed(p, LO, HI, MC, name + " " + variant)
    K = check(got, p, LO, HI, MC)
    if name == "diagonals_150":
        assert K == 75 and got.segments["n_cells"].max() == 150
    else:
        assert K == 1 and got.segments["n_cells"][0] >= 0.95 * mask.sum()


@pytest.mark.parametrize("name", ts.GIANTS)
def test_threshold_edges(name):
    _, p = ts.planes(name)
    largest = int(tr.trace(p, LO, HI, MC)[2]["n_cells"].max())
    got, _ = timed(p, LO, HI, largest, name + " min_cells = n_cells")  # keeps the segment
    assert check(got, p, LO, HI, largest) == 1 and got.segments["n_cells"][0] == largest
    got, _ = timed(p, LO, HI, largest + 1, name + " min_cells = n_cells + 1")
    assert check(got, p, LO, HI, largest + 1) == 0
    assert not got.labels.any() and got.thin.sum() >= largest
    top = float(p[3].max())
    got, _ = timed(p, LO, top, MC, name + " snr_high = max")           # one strong cell
    K = check(got, p, LO, top, MC)
    if name == "checkerboard_200":                                     # (thin == mask: the maximum is a thin cell)
        assert K == 1 and got.segments["n_strong"][0] == 1 and got.segments["snr_peak"][0] == top
    above = float(np.nextafter(top, np.inf))
    got, _ = timed(p, LO, above, MC, name + " snr_high = max + 1 ulp")
    assert check(got, p, LO, above, MC) == 0 and not got.labels.any()


def test_peak_among_tied_cells():
    """One constant snr on the whole serpentine: the peak is the smallest index of 20000 tied cells, decided across
    the lanes' strided runs and the butterfly."""
    _, p = ts.planes("serpentine_200_p2", snr_const=3.25)
    got, _ = timed(p, 1.0, 3.25, 1, "serpentine_200_p2 constant snr")
    assert check(got, p, 1.0, 3.25, 1) == 1
    s = got.segments[0]
    assert s["n_cells"] > 19000 and s["n_strong"] == s["n_cells"] and s["peak"] == s["first"] == 0


def test_one_giant_among_thousands():
    """The checkerboard's upper half, an empty row, random planes below: one key with more than 4096 entries and
    K > 256 (two radix passes) in the same sort."""
    _, top = ts.planes("checkerboard_200")
    p = np.concatenate([top[:, :100], np.zeros((4, 1, 200)), random_planes(100, 200, 11)], axis=1)
    got, _ = timed(p, 1.0, 1.0, 1, "checkerboard over random planes")
    K = check(got, p, 1.0, None, 1)
    assert K > 256 and got.segments["n_cells"].max() == 10000
    assert np.sort(got.segments["n_cells"])[-2] < 4096


def edge_planes():
    p = random_planes(257, 263, 77)
    rng = np.random.default_rng(78)
    amp, age, ang, snr = p

    def some(share=0.004):
        return rng.random(snr.shape) < share
    snr[some()] = np.inf
    snr[some()] = -np.inf
    ang[some()] = np.inf
    ang[some()] = -np.inf
    ang[some()] = 1e6
    ang[some()] = -1e6
    ang[some()] = np.nextafter(1e6, np.inf)
    ang[some()] = -np.nextafter(1e6, np.inf)
    snr[some()] = -0.0
    neg = some()
    snr[neg] = -rng.lognormal(0.0, 1.0, int(neg.sum()))
    for v in (0.5, 1.0, 4.0, 8.0):                                     # exactly snr_low and snr_high of the settings
        snr[some(0.01)] = v
    return p


def test_value_edges():
    """Infinities in snr and angle, angles at and one ulp past the 1e6 limit, -0.0 and negative snr, snr exactly at
    snr_low and at snr_high (5 % of random_planes' cells are exactly 2.0)."""
    p = edge_planes()
    assert np.isinf(p[3]).any() and np.isinf(p[2]).any() and (np.abs(p[2]) == 1e6).any() and (p[3] < 0).any()
    ks = []
    for lo, hi, mc in SETTINGS + [(2.0, 2.0, 1)]:
        got, _ = timed(p, lo, lo if hi is None else hi, mc, "value edges (%g, %s, %d)" % (lo, hi, mc))
        ks.append(check(got, p, lo, hi, mc))
    assert ks[-2] == 0 and min(ks[:-2]) > 0 and ks[-1] > 0
    # the cells past the limit are never thin, the cells at it can be
    assert not got.thin[np.abs(p[2]) > 1e6].any()
    assert sl.extract_traces(p, 0.5).thin[np.abs(p[2]) == 1e6].any()


@pytest.mark.parametrize("name", ts.GIANTS)
def test_same_bytes_every_run(name):
    _, p = ts.planes(name)
    a, _ = timed(p, LO, HI, MC, name + " again")
    b, _ = timed(p, LO, HI, MC, name + " and again")
    c = traces._traces(*_lib.Context(0).trace_planes(np.ascontiguousarray(p), LO, HI, MC))
    assert len(a.segments) == 1
    for x in (b, c):
        assert a.thin.tobytes() == x.thin.tobytes() and a.labels.tobytes() == x.labels.tobytes()
        assert a.segments.tobytes() == x.segments.tobytes()


def test_a_chain_through_1024_tiles():
    """The 1024 x 1024 serpentine, compared in full; its wall time is printed next to that of random planes of the
    same size at the same settings (profiles/trace_shapes.txt) - no ratio is asserted."""
    mask, sector = ts.serpentine(1024, 1024, 2)
    p = ts.planes_of(mask, sector, 7)
    got, _ = timed(p, LO, HI, MC, "serpentine 1024 p2")
    assert check(got, p, LO, HI, MC) == 1 and got.segments["n_cells"][0] >= 0.95 * mask.sum()
    q = random_planes(1024, 1024, 1024)
    got, _ = timed(q, LO, HI, MC, "random_planes 1024")
    assert len(got.segments) > 0
