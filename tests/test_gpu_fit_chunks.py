"""Every fit's second chunk and second round on the MI355X (option "fit_chunk", scarplet_amd/csrc/sc_fit_chunk.h).

Every fit call cuts its work into chunks on the host and strides over it in rounds on the device.  The built-in chunk
bounds (2^19 cells, 4 GiB of parked profiles, 256 MiB of cubes) and the grid caps (2048 workgroups of four cells) lie far
above the cases of the other test files, so nothing there runs the code that rebases a chunk onto the next or a wave's
second trip through its loop.  Here:

* MANY CHUNKS.  sc_set_option "fit_chunk" lowers the bound at which a driver closes a chunk and changes nothing else.
  Each of the twelve calls runs the small cases of its own test file at several bounds, through the library's Python
  binding (the raw rows, padding included), on the context's DEM and on an uploaded one, with every optional output: all
  bytes equal those of the run with the option at 0.  The launch counter (k_profile) shows that the chunks ran - for the
  segment calls it equals what the rule restated in tests/fit_chunk_reference.py gives - and at 0 it is the parent
  commit's count (PARENT_LAUNCHES), so the default path is the one it was.  One case per call, chunked, then goes through
  its family's compare function against the float64 restatement, with the family's tolerances (RTOL = 1e-9, at most 1 %
  ties): the code is not only compared with itself.
* THE SECOND ROUND.  More cells than one trip of the grid holds (3 x 8192 + 5 per-cell fits, 2 x 4096 x 4 + 5 lateral
  stations, > 8192 cells of forty segments, 65536 + 3 one-cell segments, 300 segments x 2000 replicates) on short profiles
  (h = 12, five ages).  Reference (a): the bytes of sub-calls that each stay within one trip (at most 4096 cells, whole
  segments); (b): a seeded sample - cells of the first trip, of every later one, of the last ragged round and of the
  last workgroup - against the family's restatement.  The segments of 2100 cells are left to (a): their restatement is a
  least-squares problem with 4201 columns per age, and alone in a sub-call such a segment is the shape
  tests/test_gpu_segments.py already holds against it.
* ONE CONTEXT.  The six segment calls share the sg_ buffers of a context and one driver (sc_sg_chunks) that sizes them
  from each call's description of its park: on one context, in both orders and at two sizes of the park, each call returns
  the bytes it returns on a fresh context.

Out of scope: the cap of k_st_spp / k_st_fit (65536 workgroups, 262 144 windows) and the 65536-block cap of k_bs_terms.
"""
import contextlib
import warnings

import numpy as np
import pytest

import bootstrap_reference as br
import fit_chunk_reference as fc
import lateral_reference as lr
import profile_reference as pr
import ramp_reference as rr
import robust_reference as rb
import segment_ramp_reference as sx
import segment_reference as sr
import segment_robust_reference as qr
import shift_reference as sh
import strike_reference as stk
import surface_reference as sf
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, bootstrap, core, lateral, profiles, segments, strike, surface

pytestmark = pytest.mark.gpu

PER_CELL_BOUNDS = lambda K: [1, 7, K - 1, K, K + 1]
PF_CHUNK = 1 << 19          # cells per launch of a per-cell call (sc_fit.h)
NO_BOUND = 1 << 62          # (the built-in bounds - parked bytes, segments, windows - are never reached by these cases)


# ---- plumbing ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def fit_chunk(ctx, n):
    ctx.set_option("fit_chunk", n)
    try:
        yield
    finally:
        ctx.set_option("fit_chunk", 0)


@pytest.fixture(scope="module")
def ctx(oracle_pool):
    """A context of this file's own for the binding's calls: what it holds (a DEM per case) never meets the shared one."""
    c = _lib.Context(0)
    yield c
    c.close()


def counted(ctx, call):
    """(the call's outputs, the launches it counted under k_profile)."""
    ctx.profile(0)
    out = call()
    return out, ctx.profile_get()["k_profile"][0]


def same_bytes(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert x.tobytes() == y.tobytes(), (k, x.dtype.names)


def put_dem(ctx, z, de):
    """The route on the context's DEM: a Matcher on ``ctx`` puts it there."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # (a DEM with NaN cells: the fits take it, the search would not)
        sl.Matcher(sl.DEMGrid.from_array(z, float(de)), ctx=ctx)


def both_routes(ctx, call, z, de):
    """``call(ctx, z or None)`` on the uploaded DEM and on the context's: the same bytes; returns one and its launches."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    up, n_up = counted(ctx, lambda: call(ctx, z))
    put_dem(ctx, z, de)
    own, n_own = counted(ctx, lambda: call(ctx, None))
    same_bytes(up, own)
    assert n_up == n_own
    return up, n_up


# ---- the twelve calls through the binding, every optional output asked for ---------------------------------------------
# A builder takes a case of its family's list and returns (call, K or the segments' CSR arrays): call(ctx, z) runs the
# library on the arguments the Python API would hand it
def pf_args(c):
    return profiles.check_args(c["z"].shape, c["de"], c["cells"], c["angle"], c["h"] * c["de"], c["w"] * c["de"], c["ages"],
                               c["delta"], c["min_samples"])


def sg_args(c, shift=False):
    return segments.check_args(c["z"].shape, c["de"], c["cells"], c["labels"], c["angle"], c["h"] * c["de"], c["w"] * c["de"],
                               c["ages"], c["delta"], c["min_samples"], c.get("min_profiles", 1), shift=shift)


def robust_of(c):
    kw = dict(robust=None, tuning=None, iterations=8, robust_scale=None)
    kw.update(c["robust"])
    return profiles.check_robust(c["z"].shape, c["weights"], kw["robust"], kw["tuning"], kw["iterations"], kw["robust_scale"], None)


def call_profiles(c):
    a = pf_args(c)
    return (lambda ctx, z: ctx.fit_profiles(*a, curve=True, z=z)), len(a[0])


def call_profiles_shift(c):
    a = pf_args(c)
    return (lambda ctx, z: ctx.fit_profiles(*a, curve=True, z=z, shift=c["D"], shift_plane=True)), len(a[0])


def call_profiles_ramp(c, mode):
    a = pf_args(c)
    slope = c["slope"] if mode == _lib.RAMP_SLOPE else 0.0
    return (lambda ctx, z: ctx.fit_profiles_ramp(*a, c["M"], mode=mode, slope=slope, curve=True, width_plane=True, z=z)), len(a[0])


def call_profiles_robust(c):
    a = pf_args(c)
    wt, loss, k, T, sigma = robust_of(c)
    return (lambda ctx, z: ctx.fit_profiles_robust(*a, weights=wt, loss=loss, tuning=k, iterations=T, scale=sigma, curve=True,
                                                   z=z)), len(a[0])


def call_lateral(c):
    a = lateral.check_args(c["z"].shape, c["de"], c["cells"], c["angle"], c["h"] * c["de"], c["q0"] * c["de"], c["q1"] * c["de"],
                           c["D"] * c["de"], 1.0, c["min_samples"])
    return (lambda ctx, z: ctx.lateral_offsets(*a, curve=True, z=z)), len(a[0])


class Segs(object):
    """The segment arguments of a call: ``head`` = (cells, sa, ca, seg_start, seg_label), then the call's own CSR arrays
    over the segments (``aux``: name -> array), kept apart so that empty segments can be put in."""

    def __init__(self, head, aux=None):
        self.head, self.aux = list(head), dict(aux or {})

    @property
    def seg_start(self):
        return self.head[3]

    def with_empty_segments(self, before):
        """Empty segments before the segments ``before`` (S: after the last), relabelled 1..S'."""
        out = Segs(self.head, self.aux)
        at = np.asarray(before, dtype=np.int64)
        out.head[3] = np.ascontiguousarray(np.insert(self.head[3], at, self.head[3][at]))
        out.head[4] = np.arange(1, len(out.head[3]), dtype=np.int32)
        for k, v in self.aux.items():
            out.aux[k] = np.ascontiguousarray(np.insert(v, at, v[at]))
        return out


def segs_plain(c):
    a = sg_args(c)
    g = Segs(a[:5])
    return g, lambda g: (lambda ctx, z: ctx.fit_segments(*g.head, *a[5:12], cell_table=True, curve=True, z=z))


def segs_shift(c):
    a = sg_args(c, shift=True)
    g = Segs(a[:5])
    return g, lambda g: (lambda ctx, z: ctx.fit_segments(*g.head, *a[5:12], cell_table=True, curve=True, z=z, shift=c["D"],
                                                         shift_plane=True))


def segs_ramp(c, mode):
    a = sg_args(c)
    g = Segs(a[:5])
    slope = c["slope"] if mode == _lib.RAMP_SLOPE else 0.0
    return g, lambda g: (lambda ctx, z: ctx.fit_segments_ramp(*g.head, *a[5:12], c["M"], mode=mode, slope=slope, cell_table=True,
                                                              curve=True, width_plane=True, z=z))


def segs_robust(c):
    a = sg_args(c)
    g = Segs(a[:5])
    wt, loss, k, T, sigma = robust_of(c)
    return g, lambda g: (lambda ctx, z: ctx.fit_segments_robust(*g.head, *a[5:12], weights=wt, loss=loss, tuning=k, iterations=T,
                                                                scale=sigma, cell_table=True, curve=True, z=z))


def segs_bootstrap(c, h=br.H, w=br.W):
    a = bootstrap.check_args(c["z"].shape, 1.0, c["cells"], c["labels"], c["angle"], float(h), float(w), c["block_length"],
                             c["R"], 0.95, c["seed"], c["ages"], c["min_samples"], 1, c["min_blocks"],
                             float(c["D"]) if c["D"] else None)
    g = Segs(a[:5], dict(seg_blk_start=a[5]))
    return g, lambda g: (lambda ctx, z: ctx.bootstrap_segments(*g.head, g.aux["seg_blk_start"], *a[6:], hist=True,
                                                               replicates=True, z=z))


def segs_strike(c):
    a = strike.check_args(c["z"].shape, 1.0, c["cells"], c["labels"], c["angle"], float(c["h"]), float(c["w"]), c["window"],
                          c["step"], c["ages"], c["delta"], c["min_samples"], c["min_profiles"],
                          float(c["D"]) if c["D"] else None)[0]
    g = Segs(a[:5], dict(seg_win_start=a[5]))
    return g, lambda g: (lambda ctx, z: ctx.fit_strike(*g.head, g.aux["seg_win_start"], *a[6:], curve=True, z=z))


# ---- the launches of a call, from the drivers' text -----------------------------------------------------------------------
# tables: the launches before the first chunk (the erf table, and the table of F of the ramp); of_chunk(m, items): those of
# a chunk of m cells and ``items`` of the call's own CSR array (blocks, windows).  A chunk without cells parks nothing and
# sums nothing
def launches_segments(m, items):
    return 8 if m else 2                                 # park, rank, sum1 sum2, resid, sum1 sum2, choose


def launches_robust(c):
    _, loss, _, T, sigma = robust_of(c)

    def of_chunk(m, items):
        n = 8 if m else 2                                # park, rank, sums, loss, sums, choose
        if loss != _lib.ROBUST_NONE:
            n += 1                                       # k_sq_begin
            if m and not sigma > 0.0:
                n += 16                                  # the radix select of the scale
            if m:
                n += 3 * T + 3                           # T steps with their sums, the loss with its sums
        return n
    return of_chunk


def launches_bootstrap(m, items):
    return (2 if m else 1) + (1 if items else 0) + 2     # park, rank, terms, replicates, summary


def launches_strike(m, items):
    return (2 if m else 1) + (1 if m and items else 0) + (1 if items else 0)       # park, rank, Spp, the windows' fit


def expected_launches(g, n, tables, of_chunk, aux=None):
    cuts = fc.chunks(g.seg_start, NO_BOUND, fc.bound(NO_BOUND, n))
    total = tables
    for s0, s1 in zip(cuts, cuts[1:]):
        items = 0 if aux is None else int(g.aux[aux][s1] - g.aux[aux][s0])
        total += of_chunk(int(g.seg_start[s1] - g.seg_start[s0]), items)
    return total, len(cuts) - 1


# ---- the cases ---------------------------------------------------------------------------------------------------------------
_CASES = {}


def family(name):
    """The case lists of the families' own test files, built once: the small cases only."""
    if name not in _CASES:
        make = {"profiles": lambda: {c["name"]: c for c in pr.gpu_cases(big=False)},
                "shift": lambda: {c["name"]: c for c in sh.profile_cases()},
                "ramp": lambda: {c["name"]: c for c in rr.gpu_cases()},
                "huber": lambda: rb.gpu_cases("huber"), "tukey": lambda: rb.gpu_cases("tukey"),
                "segments": lambda: {c["name"]: c for c in sr.gpu_cases()},
                "segments shift": lambda: {c["name"]: c for c in sh.segment_cases()},
                "segments ramp": lambda: {c["name"]: c for c in sx.gpu_cases()},
                "segments huber": lambda: qr.gpu_cases("huber"), "segments tukey": lambda: qr.gpu_cases("tukey"),
                "bootstrap": lambda: {c["name"]: c for c in br.gpu_cases()},
                "strike": lambda: {c["name"]: c for c in stk.gpu_cases()}}[name]
        _CASES[name] = make()
    return _CASES[name]


def lateral_case(name, K, p):
    shape, de, seed = {"96x80": ((96, 80), 1.0, 11), "129x100": ((129, 100), 2.0, 12)}[name]       # (tests/test_gpu_lateral.py)
    cells = lr.rough_stations(shape, K, 5)
    h, D, q0, q1, ms = p
    return dict(z=lr.rough_dem(shape, seed), de=de, cells=cells, angle=np.random.default_rng(K).uniform(-np.pi, np.pi, len(cells)),
                h=h, D=D, q0=q0, q1=q1, min_samples=ms)


PER_CELL = {
    "fit_profiles, synthetic h15 w2": lambda: (family("profiles")["synthetic h15 w2"], call_profiles),
    "fit_profiles, borders and corners": lambda: (family("profiles")["borders and corners"], call_profiles),
    "fit_profiles_shift, D = h - min_samples": lambda: (family("shift")["D = h - min_samples"], call_profiles_shift),
    "fit_profiles_shift, NaN cells": lambda: (family("shift")["NaN cells"], call_profiles_shift),
    "fit_profiles_ramp free, M = h - min_samples": lambda: (family("ramp")["M = h - min_samples"],
                                                            lambda c: call_profiles_ramp(c, _lib.RAMP_FREE)),
    "fit_profiles_ramp slope, h30 w5 M4": lambda: (family("ramp")["h30 w5 M4"], lambda c: call_profiles_ramp(c, _lib.RAMP_SLOPE)),
    "fit_profiles_robust huber, h15": lambda: (family("huber")["h15"], call_profiles_robust),
    "fit_profiles_robust tukey, weights: NaN cells": lambda: (family("tukey")["weights: NaN cells"], call_profiles_robust),
    "lateral_offsets, 96x80 h5 D1": lambda: (lateral_case("96x80", 257, (5, 1, 2, 9, 4)), call_lateral),
    "lateral_offsets, 129x100 h5 D32": lambda: (lateral_case("129x100", 257, (5, 32, 1, 1, 4)), call_lateral),
}

# At "fit_chunk" = 0, the launches under k_profile of every call below as the PARENT commit's library counts them (one
# run of the parent's build over these very calls): the default path issues what it issued
PARENT_LAUNCHES = {
    "fit_profiles, synthetic h15 w2": 2,
    "fit_profiles, borders and corners": 2,
    "fit_profiles_shift, D = h - min_samples": 2,
    "fit_profiles_shift, NaN cells": 2,
    "fit_profiles_ramp free, M = h - min_samples": 3,
    "fit_profiles_ramp slope, h30 w5 M4": 3,
    "fit_profiles_robust huber, h15": 2,
    "fit_profiles_robust tukey, weights: NaN cells": 2,
    "lateral_offsets, 96x80 h5 D1": 1,
    "lateral_offsets, 129x100 h5 D32": 1,
    "fit_segments, sizes 1 2 64 65 2100": 9,
    "fit_segments, shuffled order": 9,
    "fit_segments_shift, sizes 1 2 64 65 300": 9,
    "fit_segments_shift, shuffled order": 9,
    "fit_segments_ramp free, sizes 1 2 64 65 130": 10,
    "fit_segments_ramp slope, h30 w5 M4": 10,
    "fit_segments_robust huber, sizes 1 2 63 64 65 129": 38,
    "fit_segments_robust tukey, weights: NaN cells": 41,
    "bootstrap_segments, nb 1 4 5 70": 6,
    "bootstrap_segments, D 3": 6,
    "fit_along_strike, several segments": 5,
    "fit_along_strike, unusable": 5,
}


@pytest.mark.parametrize("name", list(PER_CELL))
def test_per_cell_calls_in_many_chunks(ctx, name):
    c, build = PER_CELL[name]()
    call, K = build(c)
    base, n0 = both_routes(ctx, call, c["z"], c["de"])
    assert all(v is not None for v in base) and len(base[0]) == K
    print("%s: K = %d, %d launches unchunked" % (name, K, n0))
    assert n0 == PARENT_LAUNCHES[name], (n0, PARENT_LAUNCHES[name])
    for n in PER_CELL_BOUNDS(K):
        with fit_chunk(ctx, n):
            got, launches = both_routes(ctx, call, c["z"], c["de"])
        same_bytes(got, base)
        assert launches - n0 == fc.per_cell_chunks(K, PF_CHUNK, n) - 1 == -(-K // n) - 1, (n, launches, n0)
    again, n1 = both_routes(ctx, call, c["z"], c["de"])               # the option is back at 0
    same_bytes(again, base)
    assert n1 == n0


def segment_bounds(g):
    """1, 64, 65, a value between two segment sizes, and K - 1."""
    sizes = np.unique(np.diff(g.seg_start))
    between = int(sizes[-2] + sizes[-1]) // 2 if len(sizes) > 1 else int(sizes[-1]) + 1
    return [1, 64, 65, between, int(g.seg_start[-1]) - 1]


def empties(g):
    """Empty segments first, last, in a run, and where the chunk of 65 cells closes: before and after every segment."""
    S = len(g.seg_start) - 1
    return g.with_empty_segments([0, 0] + list(range(1, S)) + [S // 2, S, S])


SEGMENT = {
    "fit_segments, sizes 1 2 64 65 2100": lambda: (family("segments")["sizes 1 2 64 65 2100"], segs_plain, 1, launches_segments, None),
    "fit_segments, shuffled order": lambda: (family("segments")["shuffled order"], segs_plain, 1, launches_segments, None),
    "fit_segments_shift, sizes 1 2 64 65 300": lambda: (family("segments shift")["sizes 1 2 64 65 300"], segs_shift, 1,
                                                        launches_segments, None),
    "fit_segments_shift, shuffled order": lambda: (family("segments shift")["shuffled order"], segs_shift, 1, launches_segments, None),
    "fit_segments_ramp free, sizes 1 2 64 65 130": lambda: (family("segments ramp")["sizes 1 2 64 65 130"],
                                                            lambda c: segs_ramp(c, _lib.RAMP_FREE), 2, launches_segments, None),
    "fit_segments_ramp slope, h30 w5 M4": lambda: (family("segments ramp")["h30 w5 M4"], lambda c: segs_ramp(c, _lib.RAMP_SLOPE), 2,
                                                   launches_segments, None),
    "fit_segments_robust huber, sizes 1 2 63 64 65 129": lambda: (family("segments huber")["sizes 1 2 63 64 65 129"], segs_robust, 1,
                                                                  "robust", None),
    "fit_segments_robust tukey, weights: NaN cells": lambda: (family("segments tukey")["weights: NaN cells"], segs_robust, 1,
                                                              "robust", None),
    "bootstrap_segments, nb 1 4 5 70": lambda: (family("bootstrap")["nb 1 4 5 70"], segs_bootstrap, 1, launches_bootstrap,
                                                "seg_blk_start"),
    "bootstrap_segments, D 3": lambda: (family("bootstrap")["D 3"], segs_bootstrap, 1, launches_bootstrap, "seg_blk_start"),
    "fit_along_strike, several segments": lambda: (family("strike")["several segments"], segs_strike, 1, launches_strike,
                                                   "seg_win_start"),
    "fit_along_strike, unusable": lambda: (family("strike")["unusable"], segs_strike, 1, launches_strike, "seg_win_start"),
}


@pytest.mark.parametrize("holes", [False, True], ids=["as it is", "with empty segments"])
@pytest.mark.parametrize("name", list(SEGMENT))
def test_segment_calls_in_many_chunks(ctx, name, holes):
    c, build, tables, of_chunk, aux = SEGMENT[name]()
    if of_chunk == "robust":
        of_chunk = launches_robust(c)
    g, bind = build(c)
    if holes:
        g = empties(g)
    call = bind(g)
    de = c.get("de", 1.0)
    base, n0 = both_routes(ctx, call, c["z"], de)
    S = len(g.seg_start) - 1
    assert all(v is not None for v in base) and len(base[0]) == (S if aux != "seg_win_start" else g.aux[aux][-1])
    print("%s: %d segments, %d cells, %d launches unchunked" % (name, S, g.seg_start[-1], n0))
    assert n0 == expected_launches(g, 0, tables, of_chunk, aux)[0]
    if not holes:
        assert n0 == PARENT_LAUNCHES[name], (n0, PARENT_LAUNCHES[name])
    cut = 0
    for n in segment_bounds(g):
        with fit_chunk(ctx, n):
            got, launches = both_routes(ctx, call, c["z"], de)
        same_bytes(got, base)
        want, chunks = expected_launches(g, n, tables, of_chunk, aux)
        assert launches == want and launches - tables >= chunks, (n, launches, want, chunks)
        assert (launches > n0) == (chunks > 1), (n, launches, n0, chunks)
        cut += chunks > 1
    assert cut >= 3                                                       # (a case of 32 cells is one chunk at 64 and 65)
    again, n1 = both_routes(ctx, call, c["z"], de)
    same_bytes(again, base)
    assert n1 == n0


# ---- the six segment calls share the sg_ buffers of one context ----------------------------------------------------------------
def shared_case(h, A):
    """96 x 80, a step along column 40 under a rough surface; segments of 1, 2, 64, 65 and 130 cells (below, at and above
    one block of the segmented sum, two blocks and a rest), shuffled.  Every family's keys, at de = 1."""
    rng = np.random.default_rng(20261022)
    z = np.cumsum(rng.standard_normal((96, 80)), 1) * 0.05 + rng.standard_normal((96, 80)) * 0.03
    z[:, 40:] += 2.0
    rows, cols = np.meshgrid(np.arange(16, 80), np.arange(30, 50), indexing="ij")
    cells = rng.choice((rows * 80 + cols).ravel(), 262, replace=False).astype(np.int64)
    wt = rng.uniform(0.5, 2.0, z.shape)
    wt[rng.random(z.shape) < 0.02] = 0.0                                 # (a weight of 0 leaves the sample out)
    return dict(z=z, de=1.0, cells=cells, labels=rng.permutation(np.repeat([1, 2, 3, 4, 5], [1, 2, 64, 65, 130])),
                angle=0.1 + 0.05 * rng.standard_normal(262), h=h, w=1, ages=10 ** np.linspace(0.0, 1.5, A), delta=1.0,
                min_samples=3, min_profiles=1, D=2, M=2, slope=0.6, weights=wt, robust=dict(robust="huber", iterations=3),
                block_length=4.0, R=20, seed=7, min_blocks=2, window=12.0, step=6.0)


SHARED_CALLS = [("plain", segs_plain), ("shift", segs_shift), ("ramp", lambda c: segs_ramp(c, _lib.RAMP_FREE)),
                ("robust", segs_robust), ("bootstrap", lambda c: segs_bootstrap(c, c["h"], c["w"])), ("strike", segs_strike)]


def test_segment_calls_share_one_context(ctx):
    """The plain, shifted, ramp, robust (with a weight plane), bootstrap and strike calls on ONE context, in that order and
    in the reverse order, each at (h, A) = (5, 5) and (15, 64) in turn, so that every call meets buffers that a smaller and
    a larger park sized - 4 planes of A columns, of A (M + 1), 9 planes and the weights, d_ci or not: each call's bytes
    are those of the same call on a fresh context.  With empty segments first, in the middle and last."""
    cases = {p: shared_case(*p) for p in ((5, 5), (15, 64))}
    calls, fresh = {}, {}
    for p, c in cases.items():
        for name, build in SHARED_CALLS:
            g, bind = build(c)
            S = len(g.seg_start) - 1
            assert sorted(np.diff(g.seg_start)) == [1, 2, 64, 65, 130]
            calls[name, p] = bind(g.with_empty_segments([0, S // 2, S]))
            own = _lib.Context(0)
            try:
                fresh[name, p] = calls[name, p](own, c["z"])
            finally:
                own.close()
            assert all(v is not None for v in fresh[name, p])
    small, large = list(cases)
    # (the parameters alternate along the calls, and then the other way round)
    order = [(name, (small, large)[(i + flip) % 2]) for flip in (0, 1) for i, (name, _) in enumerate(SHARED_CALLS)]
    for seq in (order, order[::-1]):
        for name, p in seq:
            same_bytes(calls[name, p](ctx, cases[p]["z"]), fresh[name, p])


# ---- sc_snr_surface: chunks of whole batches of cells, on the context's DEM --------------------------------------------------
def surface_call(m, c, cells):
    idx, par, ang, keep = surface.check_args((m.ny, m.nx), cells, c["params"], c["angles"], 0.1)
    arr = m.describe(getattr(sl, c["cls"]), c["scale"], par, ang)[0]
    rc = np.column_stack([idx // m.nx, idx % m.nx]).astype(np.int32)
    return lambda: m.ctx.snr_surface(arr, len(par), len(ang), rc, keep, surface=True)


def test_snr_surface_in_many_chunks():
    """The call is not counted under k_profile: a context that only ever ran the chunked call holds fewer device bytes
    than one that ran the unchunked one (the cubes are sized by the chunk)."""
    c = sf.cases()["A"]
    K = 257
    cells = np.random.default_rng(7).integers(0, c["z"].size, K)
    cells[200:] = cells[:57]                                              # repeats
    grid = sl.DEMGrid.from_array(c["z"], float(c["de"]), float(c["dy"]))
    whole = _lib.Context(0)
    base = surface_call(sl.Matcher(grid, ctx=whole), c, cells)()
    bytes_whole = whole.device_bytes()
    whole.close()
    assert all(v is not None for v in base) and base[1].shape == (K, len(c["angles"]), len(c["params"]))
    CB = _lib.SURFACE_CELL_BATCH
    for n in PER_CELL_BOUNDS(K) + [CB, CB + 1]:
        own = _lib.Context(0)
        try:
            call = surface_call(sl.Matcher(grid, ctx=own), c, cells)
            with fit_chunk(own, n):
                got = call()
            same_bytes(got, base)
            if -(-n // CB) * CB < K:                                      # more than one chunk
                assert own.device_bytes() < bytes_whole, (n, own.device_bytes(), bytes_whole)
            same_bytes(call(), base)                                      # the option is back at 0
        finally:
            own.close()
    # the chunked cubes against the float64 oracle, the table against the restatement of the cube (tests/test_gpu_surface.py)
    own = _lib.Context(0)
    try:
        m = sl.Matcher(grid, ctx=own)
        with fit_chunk(own, 7):
            tab, S, Amp = m.snr_surface(getattr(sl, c["cls"]), c["scale"], c["params"], c["angles"], cells, return_surface=True)
    finally:
        own.close()
    oS, oA, smax, amax = sf.oracle_cubes("A")
    assert (np.abs(S - oS[cells]).max(axis=0) / np.maximum(smax, 1e-300)).max() <= 1e-9
    assert (np.abs(Amp - oA[cells]).max(axis=0) / np.maximum(amax, 1e-300)).max() <= 1e-9
    want, got = sf.reduce_cube(S, Amp, 0.1), sf.table_rows(tab)
    for f in want.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), f


def test_the_option_is_checked(ctx):
    for bad in (-1, -0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\).*fit_chunk"):
            ctx.set_option("fit_chunk", bad)
    ctx.set_option("fit_chunk", 2.0 ** 70)                                # never raises a built-in bound: as good as 0
    ctx.set_option("fit_chunk", 0)


# ---- the families' restatements, behind one signature -----------------------------------------------------------------------
# run(c): the Python API's outputs of case c, every optional output asked for, on the shared context of the device;
# check(c, outs): those outputs against the family's float64 restatement of c, by the family's compare function
def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def shared_ctx():
    return core._context(0)


def rows_of(table, curve):
    return [dict({f: table[f][k] for f in table.dtype.names}, curve=curve[k]) for k in range(len(table))]


def by_input_position(c, cell_table):
    kept = np.flatnonzero(c["labels"] > 0)
    assert len(cell_table) == len(kept) and np.array_equal(cell_table["cell"], c["cells"][kept])
    full = np.zeros(len(c["cells"]), dtype=cell_table.dtype)
    full[kept] = cell_table
    return full


def api_profiles(c, **kw):
    return sl.fit_profiles(grid(c["z"], c["de"]), c["cells"], c["angle"], c["h"] * c["de"], c["w"] * c["de"], ages=c["ages"],
                           delta=c["delta"], min_samples=c["min_samples"], return_curve=True, **kw)


def api_segments(c, **kw):
    return sl.fit_segments(grid(c["z"], c["de"]), c["cells"], c["labels"], c["angle"], c["h"] * c["de"], c["w"] * c["de"],
                           ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"], min_profiles=c.get("min_profiles", 1),
                           return_cells=True, return_curve=True, **kw)


def check_plain(c, outs):
    idx, ref = pr.restate(dict(c, sample=None))
    return pr.compare_rows(ref, rows_of(*outs), c["h"], c["de"], c["delta"])


def check_shift(c, outs):
    ref = sh.fit_profiles(c["z"], c["de"], c["cells"], c["angle"], c["h"], c["w"], c["D"], c["ages"], c["delta"], c["min_samples"])
    return sh.compare_rows(ref, *outs, c["h"], c["de"], c["D"], c["delta"])


def check_ramp(mode):
    def check(c, outs):
        return rr.compare_rows(rr.restate(c, mode), *outs, c["h"], c["de"], c["M"], mode, c["slope"], c["delta"])
    return check


def check_robust(c, outs):
    return rb.compare_rows(c, rb.restate(c), rows_of(*outs))


def ramp_kw(mode):
    return lambda c: dict(max_width=c["M"] * c["de"], initial_slope=c["slope"] if mode == rr.SLOPE else None, return_width=True)


PROFILE_FAMILIES = {
    "plain": (lambda c: {}, check_plain),
    "shift": (lambda c: dict(max_shift=c["D"] * c["de"], return_shift=True), check_shift),
    "ramp free": (ramp_kw(rr.FREE), check_ramp(rr.FREE)),
    "ramp slope": (ramp_kw(rr.SLOPE), check_ramp(rr.SLOPE)),
    "robust": (lambda c: dict(weights=c["weights"], **c["robust"]), check_robust),
}


def seg_check_plain(c, outs):
    table, cells, curve = outs
    return sr.compare(sr.restate(c), table, by_input_position(c, cells), curve, c["h"], c["de"], c["delta"])


def seg_check_shift(c, outs):
    """Stage one's d_ci against the single-profile restatement, then the joint fit with those shifts
    (tests/test_gpu_shift.py)."""
    table, cells, curve, shifts = outs
    single = sh.fit_profiles(c["z"], c["de"], c["cells"], c["angle"], c["h"], c["w"], c["D"], c["ages"], c["delta"], c["min_samples"])
    ties = 0
    for k, r in enumerate(single):
        if r["usable"]:
            assert r["cond"] <= sh.COND_MAX, (r["cell"], r["cond"])
            ties += sh.check_shifts(r, shifts[k]) > 0
        else:
            assert not shifts[k].any()
    assert ties <= sh.TIE_SHARE * max(1, len(single)), ties
    ref = sh.fit_segments(c["z"], c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"], c["D"], c["ages"], shifts, c["delta"],
                          c["min_samples"], c.get("min_profiles", 1))
    return sh.compare_segments(ref, table, by_input_position(c, cells), curve, c["h"], c["de"], c["D"], c["delta"])


def seg_check_ramp(mode):
    def check(c, outs):
        table, cells, curve, widths = outs
        return sx.compare_segments(sx.restate(c, mode), table, by_input_position(c, cells), curve, widths, c["h"], c["de"], c["M"],
                                   mode, c["slope"], c["delta"])
    return check


def seg_check_robust(c, outs):
    table, cells, curve = outs
    return qr.compare(c, qr.restate(c), table, by_input_position(c, cells), curve)


SEGMENT_FAMILIES = {
    "plain": (lambda c: {}, seg_check_plain),
    "shift": (lambda c: dict(max_shift=c["D"] * c["de"], return_shift=True), seg_check_shift),
    "ramp free": (ramp_kw(sx.FREE), seg_check_ramp(sx.FREE)),
    "ramp slope": (ramp_kw(sx.SLOPE), seg_check_ramp(sx.SLOPE)),
    "robust": (lambda c: dict(weights=c["weights"], **c["robust"]), seg_check_robust),
}


def api_bootstrap(c):
    return sl.bootstrap_segments(grid(c["z"], 1.0), c["cells"], c["labels"], c["angle"], float(c.get("h", br.H)),
                                 float(c.get("w", br.W)), block_length=c["block_length"], replicates=c["R"], seed=c["seed"],
                                 ages=c["ages"], min_samples=c["min_samples"], min_blocks=c["min_blocks"],
                                 max_shift=float(c["D"]) if c["D"] else None, return_hist=True, return_replicates=True)


def check_bootstrap(c, outs):
    ref = br.bootstrap_segments(c["z"], 1.0, c["cells"], c["labels"], c["angle"], c.get("h", br.H), c.get("w", br.W), c["ages"],
                                c["block_length"], c["R"], 0.95, c["seed"], c["D"], c["min_samples"], 1, c["min_blocks"])
    return br.compare(ref, *outs)


def api_strike(c):
    return sl.fit_along_strike(grid(c["z"], 1.0), c["cells"], c["labels"], c["angle"], float(c["h"]), float(c["w"]),
                               window=c["window"], step=c["step"], ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"],
                               min_profiles=c["min_profiles"], return_curve=True)


def check_strike(c, outs):
    assert not c["D"]
    return stk.compare(stk.restate(c), *outs, c["ages"], c["delta"])


def api_lateral(c):
    return sl.lateral_offsets(grid(c["z"], c["de"]), c["cells"], c["angle"], c["h"] * c["de"], c["q0"] * c["de"], c["q1"] * c["de"],
                              c["D"] * c["de"], min_samples=c["min_samples"], return_curve=True)


def check_lateral(c, outs):
    from test_gpu_lateral import assert_no_near_ties, compare           # (the family's compare function lives there)
    ref = lr.lateral_offsets(c["z"], c["de"], c["cells"], c["angle"], c["h"], c["q0"], c["q1"], c["D"], 1.0, c["min_samples"])
    assert_no_near_ties(*ref)
    return compare(ref, *outs)


# ---- many chunks, against the restatement: one case per call --------------------------------------------------------------
RESTATED = {
    "fit_profiles": lambda: (family("profiles")["synthetic h15 w2"], 7, lambda c: api_profiles(c), check_plain),
    "fit_profiles_shift": lambda: (family("shift")["D = h - min_samples"], 7,
                                   lambda c: api_profiles(c, **PROFILE_FAMILIES["shift"][0](c)), check_shift),
    "fit_profiles_ramp free": lambda: (family("ramp")["M = h - min_samples"], 7,
                                       lambda c: api_profiles(c, **ramp_kw(rr.FREE)(c)), check_ramp(rr.FREE)),
    "fit_profiles_ramp slope": lambda: (family("ramp")["M = h - min_samples"], 7,
                                        lambda c: api_profiles(c, **ramp_kw(rr.SLOPE)(c)), check_ramp(rr.SLOPE)),
    "fit_profiles_robust huber": lambda: (family("huber")["h15"], 7, lambda c: api_profiles(c, **PROFILE_FAMILIES["robust"][0](c)),
                                          check_robust),
    "fit_profiles_robust tukey": lambda: (family("tukey")["weights: NaN cells"], 7,
                                          lambda c: api_profiles(c, **PROFILE_FAMILIES["robust"][0](c)), check_robust),
    "lateral_offsets": lambda: (lateral_case("96x80", 257, (5, 1, 2, 9, 4)), 7, api_lateral, check_lateral),
    "fit_segments": lambda: (family("segments")["synthetic h15 w2"], 65, lambda c: api_segments(c), seg_check_plain),
    "fit_segments_shift": lambda: (family("segments shift")["sizes 1 2 64 65 300"], 65,
                                   lambda c: api_segments(c, **SEGMENT_FAMILIES["shift"][0](c)), seg_check_shift),
    "fit_segments_ramp free": lambda: (family("segments ramp")["sizes 1 2 64 65 130"], 65,
                                       lambda c: api_segments(c, **ramp_kw(sx.FREE)(c)), seg_check_ramp(sx.FREE)),
    "fit_segments_ramp slope": lambda: (family("segments ramp")["sizes 1 2 64 65 130"], 65,
                                        lambda c: api_segments(c, **ramp_kw(sx.SLOPE)(c)), seg_check_ramp(sx.SLOPE)),
    "fit_segments_robust huber": lambda: (family("segments huber")["sizes 1 2 63 64 65 129"], 65,
                                          lambda c: api_segments(c, **SEGMENT_FAMILIES["robust"][0](c)), seg_check_robust),
    "fit_segments_robust tukey": lambda: (family("segments tukey")["sizes 1 2 63 64 65 129"], 65,
                                          lambda c: api_segments(c, **SEGMENT_FAMILIES["robust"][0](c)), seg_check_robust),
    "bootstrap_segments": lambda: (family("bootstrap")["nb 1 4 5 70"], 65, api_bootstrap, check_bootstrap),
    "fit_along_strike": lambda: (family("strike")["several segments"], 65, api_strike, check_strike),
}


@pytest.mark.parametrize("name", list(RESTATED))
def test_chunked_runs_against_the_restatement(name):
    c, n, run, check = RESTATED[name]()
    ctx = shared_ctx()
    ctx.profile(0)
    with fit_chunk(ctx, n):
        outs = run(c)
    chunked = ctx.profile_get()["k_profile"][0]
    st = check(c, outs)
    ctx.profile(0)
    again = run(c)
    print("%s at fit_chunk = %d: %s; %d launches for %d" % (name, n, st, chunked, ctx.profile_get()["k_profile"][0]))
    assert chunked > ctx.profile_get()["k_profile"][0]                    # the chunks ran
    same_bytes(outs, again)


# ---- the second round ----------------------------------------------------------------------------------------------------------
H2, W2, D2, M2 = 12, 1, 2, 2
AGES2 = _plan.age_grid()[:25:5]                                           # five young ages: 1 .. 100, bent over 25 points
TRIP = 4 * 2048                                                           # cells a trip of the grid of a wave-per-cell kernel holds
SUB = 4096                                                                # cells of a sub-call: half a trip


def round_sample(K, per_wg, grid_cap, count, seed):
    """``count`` sorted positions of 0..K-1, seeded: the first and last of every trip of a grid of ``grid_cap`` workgroups
    of ``per_wg`` items, the items of the last - ragged - round and of the last workgroup of every trip, the rest drawn
    evenly over the trips."""
    trip = per_wg * grid_cap
    trips = -(-K // trip)
    assert trips >= 2
    pick = set(range((K - 1) // per_wg * per_wg, K))
    for t in range(trips):
        lo, hi = t * trip, min(K, (t + 1) * trip)
        pick.update([lo, hi - 1])
        pick.update(range(min(K, lo + (grid_cap - 1) * per_wg), min(K, lo + grid_cap * per_wg)))
    assert len(pick) <= count
    rng = np.random.default_rng(seed)
    share = (count - len(pick)) // trips
    for t in list(range(trips)) + [None]:                                  # (None: what is still missing, from anywhere)
        lo, hi = (0, K) if t is None else (t * trip, min(K, (t + 1) * trip))
        free = np.setdiff1d(np.arange(lo, hi), np.fromiter(pick, dtype=np.int64))
        pick.update(rng.choice(free, min(share if t is not None else count - len(pick), len(free)), replace=False).tolist())
    out = np.array(sorted(pick), dtype=np.int64)
    assert len(out) == min(count, K)
    assert all(((out >= t * trip) & (out < (t + 1) * trip)).sum() >= 3 for t in range(trips))
    return out


_SECOND = {}


def second_round_cells(K, seed, margin=20):
    """K cells of synthetic_z(600): the interior, where every profile is whole, and - one in sixteen - the first three
    columns, where the profile has nothing on one side and the cell is not fitted."""
    rng = np.random.default_rng(seed)
    rows, cols = rng.integers(margin, 600 - margin, K), rng.integers(margin, 600 - margin, K)
    edge = rng.random(K) < 1.0 / 16
    cols[edge] = rng.integers(0, 3, int(edge.sum()))
    return rows * 600 + cols, 0.2 + 0.05 * rng.standard_normal(K)


def profile_case(which):
    """The second-round cases of the per-cell calls (each built once)."""
    which = "profiles, " + which
    if which not in _SECOND:
        z = pr.synthetic_z(600)
        if which == "profiles, table in global memory":
            # 129 rows of 64 ages are 66 048 bytes: past the 65 536 up to which the kernels stage the erf table in LDS
            cells, angle = second_round_cells(TRIP + 5, 20261022, margin=70)
            c = dict(z=z, cells=cells, angle=angle, h=62, w=1, D=2, ages=10 ** np.linspace(0, 3.0, 64), min_samples=15)
        else:
            cells, angle = second_round_cells(3 * TRIP + 5, 20261021)
            c = dict(z=z, cells=cells, angle=angle, h=H2, w=W2, D=D2, M=M2, slope=0.3, ages=AGES2, min_samples=4)
        wt = np.random.default_rng(5).uniform(0.2, 3.0, z.shape) if which == "profiles, weight plane" else None
        robust = {"profiles, huber": dict(robust="huber", iterations=3),
                  "profiles, tukey": dict(robust="tukey", iterations=3)}.get(which, {})
        _SECOND[which] = dict(c, name="second round, " + which, de=1.0, delta=1.0, weights=wt, robust=robust,
                              cells=np.ascontiguousarray(cells, dtype=np.int64), angle=np.ascontiguousarray(angle))
    return _SECOND[which]


def take_cells(c, idx, tag):
    return dict(c, name="%s, %s" % (c["name"], tag), cells=np.ascontiguousarray(c["cells"][idx]),
                angle=np.ascontiguousarray(c["angle"][idx]))


def concatenated(parts):
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(len(parts[0])))


SECOND_PROFILES = [("plain", "plain", "plain"), ("shift", "shift", "shift"), ("ramp free", "ramp free", "ramp"),
                   ("ramp slope", "ramp slope", "ramp"), ("robust huber", "robust", "huber"), ("robust tukey", "robust", "tukey"),
                   ("weight plane", "robust", "weight plane"), ("shift, table in global memory", "shift", "table in global memory")]


@pytest.mark.parametrize("name,fam,which", SECOND_PROFILES, ids=[p[0] for p in SECOND_PROFILES])
def test_second_round_of_the_per_cell_kernels(name, fam, which):
    c = profile_case(which)
    kw, check = PROFILE_FAMILIES[fam]
    K = len(c["cells"])
    assert K > TRIP and K % 4
    outs = api_profiles(c, **kw(c))
    assert (outs[0]["status"] == 1).sum() > K // 32 and (outs[0]["status"] != 1).sum() > K // 2
    # (a) the bytes of sub-calls that stay within half a trip of the grid
    parts = [api_profiles(take_cells(c, slice(k0, k0 + SUB), "sub-call"), **kw(c)) for k0 in range(0, K, SUB)]
    same_bytes(outs, concatenated(parts))
    # (b) a sample of every trip against the restatement (100 cells where a cell costs 64 ages x 5 shifts of 125 points)
    idx = round_sample(K, 4, 2048, 100 if which == "table in global memory" else 300, 11)
    st = check(take_cells(c, idx, "sample"), tuple(o[idx] for o in outs))
    print("%s: %d cells, %d sampled: %s" % (name, K, len(idx), st))


def test_second_round_of_the_lateral_kernel():
    waves, cap = 4, 4096                                                   # (what lt_run gives this shape, and LT_MAX_GRID)
    K = 2 * cap * waves + 5
    c = lateral_case("96x80", K, (5, 1, 2, 9, 4))
    outs = api_lateral(c)
    parts = [api_lateral(take_cells(dict(c, name="lateral"), slice(k0, k0 + SUB), "sub-call")) for k0 in range(0, K, SUB)]
    same_bytes(outs, concatenated(parts))
    idx = round_sample(K, waves, cap, 300, 12)
    worst = check_lateral(take_cells(dict(c, name="lateral"), idx, "sample"), tuple(o[idx] for o in outs))
    print("lateral_offsets: %d stations, %d sampled, worst relative difference %.2e" % (K, len(idx), worst))


# the segment kernels: forty-odd segments of 1, 2, 64, 65, 130 and 2100 cells, more than a trip's cells in one chunk, the
# last of them small - and 65536 + 3 segments of one cell: past the caps of the grids that stride over segments and blocks
def segment_case(which):
    which = "segments, " + which
    if which not in _SECOND:
        z = pr.synthetic_z(600)
        rng = np.random.default_rng(20261023)
        if which == "segments, forty segments":
            sizes = [2100] + [1, 2, 64, 65, 130] * 3 + [2100] + [130, 65, 64, 2, 1] * 2 + [2100] + [64, 130, 1, 65, 2] * 2 \
                + [130, 130, 65, 64, 2, 1]
        else:
            sizes = [1] * (65536 + 3)
        K = sum(sizes)
        lab = np.repeat(np.arange(1, len(sizes) + 1), sizes)
        cells = pr.scarp_cells(600, K, rng, spread=1.0)
        angle = 0.2 + 0.02 * rng.standard_normal(K)
        perm = rng.permutation(K)
        _SECOND[which] = dict(name="second round, " + which, z=z, de=1.0, cells=np.ascontiguousarray(cells[perm]),
                              labels=np.ascontiguousarray(lab[perm]), angle=np.ascontiguousarray(angle[perm]), h=H2, w=W2, D=D2,
                              M=M2, slope=0.3, ages=AGES2, delta=1.0, min_samples=4, min_profiles=1, weights=None,
                              robust=dict(robust="huber", iterations=2), sizes=np.array(sizes))
    return _SECOND[which]


def take_segments(c, labels, tag):
    keep = np.isin(c["labels"], labels)
    return dict(c, name="%s, %s" % (c["name"], tag), cells=np.ascontiguousarray(c["cells"][keep]),
                labels=np.ascontiguousarray(c["labels"][keep]), angle=np.ascontiguousarray(c["angle"][keep])), keep


def segment_outputs_of(c, outs, labels, keep, fam):
    """The rows of the segments ``labels`` in the outputs of the whole call: per segment (table, curve, widths) by label, per
    cell (cell table, shifts) by input position."""
    seg = np.isin(outs[0]["label"], labels)
    per_cell = (False, True, False, True) if fam == "shift" else (False, True, False, False)
    return tuple(o[keep] if pc else o[seg] for o, pc in zip(outs, per_cell))


def sub_calls(sizes, most):
    """Runs of whole segments (1-based labels, in order) of at most ``most`` cells each."""
    runs, cur, n = [], [], 0
    for s, size in enumerate(sizes):
        if cur and n + size > most:
            runs.append(cur)
            cur, n = [], 0
        cur.append(s + 1)
        n += size
    return runs + [cur]


@pytest.mark.parametrize("fam", ["plain", "shift", "ramp free", "robust"])
@pytest.mark.parametrize("which", ["forty segments", "one-cell segments"])
def test_second_round_of_the_segment_kernels(which, fam):
    c = segment_case(which)
    kw, check = SEGMENT_FAMILIES[fam]
    sizes = c["sizes"]
    S, K = len(sizes), int(sizes.sum())
    assert K > TRIP and (which == "forty segments" or S > 65536)
    outs = api_segments(c, **kw(c))
    assert len(outs[0]) == S and (outs[0]["status"] != 1).sum() > S // 2
    # (a) the bytes of sub-calls of whole segments that stay within half a trip
    for labels in sub_calls(sizes, SUB):
        sub, keep = take_segments(c, labels, "sub-call")
        same_bytes(api_segments(sub, **kw(c)), segment_outputs_of(c, outs, labels, keep, fam))
    # (b) sampled segments against the restatement
    if which == "forty segments":
        first = np.cumsum(sizes) - sizes                                  # each segment's first cell in the chunk
        big = np.flatnonzero(sizes == 130)
        late = big[first[big] + 130 > TRIP]                               # (the segments of 130 cells at and after the trip's end)
        assert len(late) >= 1 and (first[sizes <= 65] > TRIP).sum() >= 3
        pick = np.concatenate([np.flatnonzero(sizes <= 65), late[:1]]) + 1
    else:
        pick = np.union1d(round_sample(S, 1, 65536, 40, 13), round_sample(S, 4, 2048, 60, 14)) + 1
    sub, keep = take_segments(c, pick, "sample")
    st = check(sub, segment_outputs_of(c, outs, pick, keep, fam))
    print("%s, %s: %d segments, %d cells, %d segments sampled: %s" % (which, fam, S, K, len(pick), st))


def bootstrap_case(which):
    which = "bootstrap, " + which
    if which not in _SECOND:
        z = pr.synthetic_z(600, sigma=0.3)
        rng = np.random.default_rng(20261024)
        if which == "bootstrap, 300 segments":
            sizes, R = [12] * 300, 1999                                    # 300 x 32 tiles of 64 replicates: 9600 work items
        else:
            sizes, R = [1] * (65536 + 3), 63
        K = sum(sizes)
        lab = np.repeat(np.arange(1, len(sizes) + 1), sizes)
        perm = rng.permutation(K)
        _SECOND[which] = dict(name="second round, " + which, z=z, cells=pr.scarp_cells(600, K, rng, spread=1.0)[perm],
                              labels=lab[perm], angle=(0.2 + 0.02 * rng.standard_normal(K))[perm], h=H2, w=W2, D=0, ages=AGES2,
                              block_length=25.0, R=R, seed=7, min_blocks=5, min_samples=4, sizes=np.array(sizes))
    return _SECOND[which]


@pytest.mark.parametrize("which", ["300 segments", "one-cell segments"])
def test_second_round_of_the_bootstrap_kernels(which):
    c = bootstrap_case(which)
    S = len(c["sizes"])
    tiles = -(-(c["R"] + 1) // 64)
    assert S * tiles > 8192                                               # BS_MAX_GRID
    outs = api_bootstrap(c)
    booted = int((outs[0]["status"] != 1).sum())
    assert len(outs[0]) == S and (booted > S // 2 if which == "300 segments" else booted == 0)
    # (a) sub-calls within one trip of every grid: at most 100 segments of 12 cells, or 4096 of one
    step = 100 if which == "300 segments" else SUB
    for s0 in range(0, S, step):
        labels = np.arange(s0 + 1, min(S, s0 + step) + 1)
        sub, keep = take_segments(c, labels, "sub-call")
        same_bytes(api_bootstrap(sub), tuple(o[s0:s0 + step] for o in outs))
    # (b) 100 segments of every trip against the restatement (the streams are keyed by the label: they do not move)
    per = 8192 // tiles if which == "300 segments" else 8192
    pick = round_sample(S, 1, per, 100, 15) + 1
    sub, keep = take_segments(c, pick, "sample")
    st = check_bootstrap(sub, tuple(o[pick - 1] for o in outs))
    print("bootstrap, %s: %d segments, %d bootstrapped, %d sampled: %s" % (which, S, booted, len(pick), st))
