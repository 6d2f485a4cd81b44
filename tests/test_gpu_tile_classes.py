"""Every kernel class of the FFT path's dispatch table against the float64 oracle, by forced tile plans.

The route (fft_route, scarplet_amd/csrc/sc_fft_route.h) chooses the kernels by the tile's column length Ty (64 .. 256: k_inv_cols_sym or the generic k_inv_cols;
512: k_inv_cols_symx / k_inv_cols_h2 / the paired-orientation form; 1024, 2048: the wave-per-column kernels with the
fused forward column transform; 4096: the generic complex path, no symmetric-template kernel there), by the row length Tx (512,
1024, 2048: k_inv_rows_fast and its near-tie and dealt-out forms; the rest: k_inv_rows), by the chunk's parity and masks,
by the parity of the tile count (an odd count sends the last tile through the paired-template chunk) and by whether maps
or the fold are asked for.  A natural plan on the suite's DEMs reaches a few of these combinations; a hand-built plan
(tests/tile_plans.py) puts tiles of any size and number on a 150 x 131 DEM - on the periodic whole-DEM context the tile
loads index modulo the DEM, and sc_match accepts any plan whose tiles cover the core - so one oracle stack per (DEM,
template family) serves all 49 (Ty, Tx) pairs.

Families: Scarp (parity 1), Ricker (parity 2), LeftFacingUpperBreakScarp (the Scarp window with per-cell error masks:
parity 1 and `full_masks`), and the same UpperBreak descriptors with their support boxes widened by one row, which no
longer map onto themselves under the flip: parity 0, the generic complex path at EVERY column length (what a plugin's
host-uploaded windows take).  The widened box holds the same window - the added row lies outside the support - so the
oracle stack is the UpperBreak one.

The tolerances are the project's own (oracle.PARITY, snr_tolerance, tie_window) and the policy is report()'s: no cell
outside the tolerances, no cell off the oracle's argmax, the measured SNR error at most half the tie window.  Every
plan prints one line in report()'s format (pytest -s) with its measured snr_err and amp_err; profiles/tile_classes.txt
holds those lines as measured, with the build id of the library that gave them.
"""
import numpy as np
import pytest

import scarplet_oracle as orc
import scarplet_amd as sl
from scarplet_amd import _plan, synthetic
from scarplet_amd import WindowedTemplate as WT
from parity_report import report
from tile_plans import SIZES, forced_plan, count_with_parity

pytestmark = pytest.mark.gpu

P_AMP = orc.PARITY["amp"]
ANGLES = np.linspace(-1.2, 1.2, 5)
GROUP = 3
# name -> (class, oracle kind, scale, parameters, support boxes widened by a row)
FAMILIES = {
    "scarp": (WT.Scarp, orc.SCARP, 12, (2.0, 10.0, 50.0), False),
    "ricker": (WT.Ricker, orc.RICKER, 8, (1.0, 2.0, 4.0), False),
    "upper": (WT.LeftFacingUpperBreakScarp, orc.LEFT_UPPER, 12, (2.0, 10.0, 50.0), False),
    "upper-p0": (WT.LeftFacingUpperBreakScarp, orc.LEFT_UPPER, 12, (2.0, 10.0, 50.0), True),
}
_DEMS, _STACKS = {}, {}


def dem(name):
    """DEM "A": 150 x 131 (even ny, odd nx); "B": 151 x 130, the other parity of both axes - the parities set the
    offsets oy / ox of the tile origins and the phase tables of the symmetric-template path.  Default noise: both have
    a noise floor."""
    if name not in _DEMS:
        _DEMS[name] = synthetic.synthetic_scarp(131, seed=11, ny=150) if name == "A" else \
            synthetic.synthetic_scarp(130, seed=12, ny=151)
    return _DEMS[name]


def oracle_stack(name, kind, scale, params, angles):
    """orc.snr_stack of a case as (T, ny, nx) stacks in descriptor-id order with every template's (parameter, angle):
    computed once per session, read only."""
    key = (name, kind, scale, tuple(params), tuple(np.asarray(angles, float)))
    if key not in _STACKS:
        g = dem(name)
        z = np.asarray(g._griddata, dtype=float)
        a_st, s_st = orc.snr_stack(z, float(g._georef_info.dx), float(g._georef_info.dy), kind, scale, list(params), angles)
        T = len(params) * len(angles)
        out = (a_st.reshape((T,) + z.shape), s_st.reshape((T,) + z.shape),
               np.repeat(np.asarray(params, float), len(angles)), np.tile(np.asarray(angles, float), len(params)))
        for a in out:
            a.setflags(write=False)
        _STACKS[key] = out
    return _STACKS[key]


def described(m, family, params=None, angles=ANGLES):
    """(descriptors, support box) of a family on the matcher's DEM; the supports stay below the smallest tile."""
    cls, kind, scale, par, widen = FAMILIES[family]
    par = par if params is None else params
    arr, bbox, _ = m.describe(cls, scale, np.asarray(par, float), np.asarray(angles, float))
    if widen:
        # (the library evaluates the analytic window over the box, templ_from_descriptor: the added row lies outside
        #  the support, so it holds zeros by construction - the host model's widened case checks that against the oracle)
        for k in range(len(arr)):
            arr[k].pmin -= 1
        bbox = (bbox[0] - 1,) + tuple(bbox[1:])
    assert bbox[1] - bbox[0] < 64 and bbox[3] - bbox[2] < 64, (family, bbox)
    return arr, bbox


def check(res, name, family, params=None, angles=ANGLES):
    _, kind, scale, par, _ = FAMILIES[family]
    a_st, s_st, p_of, a_of = oracle_stack(name, kind, scale, par if params is None else params, angles)
    rtol, afac = orc.snr_tolerance(kind)
    return orc.check_fold(res, a_st, s_st, p_of, a_of, tie_rtol=orc.tie_window("fft", kind),
                          amp_tol=(P_AMP[0], P_AMP[1] * np.max(np.abs(a_st))), snr_tol=(rtol, afac * np.max(s_st)))


def run_fold(gpu_ctx, name, family, Ty, Tx, nty=None, ntx=None):
    """One forced plan through sc_match from a fresh record, checked against the oracle by report()'s policy."""
    g = dem(name)
    m = sl.Matcher(g, ctx=gpu_ctx)
    arr, bbox = described(m, family)
    f = forced_plan(m.ny, m.nx, bbox, Ty, Tx, nty, ntx, group=GROUP)
    par = FAMILIES[family][3]
    gpu_ctx.reset_best()
    gpu_ctx.match(arr, sl._lib.sc_plan(**f))
    res = gpu_ctx.get_result(np.repeat(np.asarray(par, float), len(ANGLES)), np.tile(ANGLES, len(par)))
    chk = check(res, name, family)
    label = "%s %s Ty=%d Tx=%d nty=%d ntx=%d" % (name, family, Ty, Tx, f["nty"], f["ntx"])
    assert chk["n_bad"] == 0, (label, chk["n_bad"], np.argwhere(~chk["ok"])[:5])
    report(label, chk, "fft")
    return f


# 4096 x 4096: 16.8 M cells per tile and template.  All four families run there; nothing is left out.
@pytest.mark.parametrize("Ty", SIZES)
def test_fold_matrix(gpu_ctx, Ty):
    """(a) every (Ty, Tx) with the smallest tile count, DEM A, every family.  From 256 upwards that is ONE tile: an odd
    count, so the symmetric families' tile goes through the paired-template chunk where the row kernel is the fast one."""
    for family in FAMILIES:
        for Tx in SIZES:
            f = run_fold(gpu_ctx, "A", family, Ty, Tx)
            assert Ty < 256 or f["nty"] == 1
            assert Tx < 256 or f["ntx"] == 1


@pytest.mark.parametrize("Ty", SIZES)
def test_fold_tile_counts(gpu_ctx, Ty):
    """(a) an even number of tiles (whole tile pairs, no paired-template chunk: two rows of tiles, or the smallest even
    number that covers the DEM) with Tx of the slow, the fast and the widest row kernel; and an odd number above one on
    the diagonal (three rows, or the smallest odd numbers that cover: pairs, then a paired-template chunk)."""
    g = dem("A")
    for family in FAMILIES:
        bbox = described(sl.Matcher(g, ctx=gpu_ctx), family)[1]
        span_y, span_x = bbox[1] - bbox[0], bbox[3] - bbox[2]
        for Tx in (64, 512, 4096):
            nty = count_with_parity(150, span_y, Ty, 2, odd=False)
            f = run_fold(gpu_ctx, "A", family, Ty, Tx, nty=nty)
            assert (f["nty"] * f["ntx"]) % 2 == 0 and (Ty < 256 or f["nty"] == 2)
        nty = count_with_parity(150, span_y, Ty, 3, odd=True)
        ntx = count_with_parity(131, span_x, Ty, 1, odd=True)
        f = run_fold(gpu_ctx, "A", family, Ty, Ty, nty=nty, ntx=ntx)
        assert (f["nty"] * f["ntx"]) % 2 == 1 and f["nty"] >= 3 and (Ty < 256 or (f["nty"], f["ntx"]) == (3, 1))


@pytest.mark.parametrize("Ty", SIZES)
def test_fold_other_parity(gpu_ctx, Ty):
    """(a) DEM B, odd ny and even nx: the diagonal, and the four corners of the matrix."""
    for family in FAMILIES:
        for Tx in sorted({Ty} | ({64, 4096} if Ty in (64, 4096) else set())):
            run_fold(gpu_ctx, "B", family, Ty, Tx)


MAPS = [(T, T) for T in SIZES] + [(64, 4096), (4096, 64), (2048, 64)]


@pytest.mark.parametrize("Ty,Tx", MAPS)
def test_single_template_maps(gpu_ctx, Ty, Tx):
    """(b) sc_match_template (`to_maps`: every cell written, no row skipping, no orientation batching, never the fused
    forward column transform) against the oracle's maps of the same template, PARITY's value tolerances."""
    g = dem("A")
    m = sl.Matcher(g, ctx=gpu_ctx)
    for family in ("scarp", "upper"):
        arr, bbox = described(m, family)
        a_st, s_st, p_of, a_of = oracle_stack("A", *FAMILIES[family][1:4], ANGLES)
        assert (p_of[0], a_of[0]) == (FAMILIES[family][3][0], ANGLES[0])              # (descriptor 0: id 0)
        f = forced_plan(m.ny, m.nx, bbox, Ty, Tx, group=1)
        amp, snr = gpu_ctx.match_template(arr[0], sl._lib.sc_plan(**f))
        o_amp, o_snr = a_st[0], s_st[0]
        rtol, afac = orc.snr_tolerance(FAMILIES[family][1])
        ea = np.abs(amp - o_amp) - (P_AMP[0] * np.abs(o_amp) + P_AMP[1] * np.max(np.abs(o_amp)))
        es = np.abs(snr - o_snr) - (rtol * np.abs(o_snr) + afac * np.max(o_snr))
        print("maps %s Ty=%d Tx=%d: max |d amp| %.2e of %.2e, max |d snr| %.2e of %.2e" %
              (family, Ty, Tx, np.max(np.abs(amp - o_amp)), np.max(np.abs(o_amp)), np.max(np.abs(snr - o_snr)), np.max(o_snr)))
        assert (ea <= 1e-30).all() and (es <= 1e-30).all(), (family, Ty, Tx, float(ea.max()), float(es.max()))


# ---- (c) the exact mode ------------------------------------------------------------------------------------------
def _paired_angles():
    """every 45th orientation of the grid twice, 2e-5 rad apart (near-ties inside the float32 error), the grid's end
    twins -pi/2 and +pi/2 first and last"""
    grid = _plan.angle_grid(-np.pi / 2, np.pi / 2)
    base = grid[:-1:45]
    return np.concatenate([base, base[1:] + 2e-5, grid[-1:]])


EXACT = {"scarp": (2.0, 4.0, 4.0004, 50.0), "ricker": (1.0, 4.0, 4.0003)}
FAST_TX = (512, 1024, 2048)


@pytest.mark.parametrize("Ty", SIZES)
def test_exact_mode(gpu_ctx, Ty):
    """(c) the near-tie flags of the fast row kernel and the float64 settle, for every column kernel: twin orientations
    2e-5 rad apart and a repeated age - the float32 search cannot order them, the settled record carries the oracle's
    argmax in every cell (the grid's end twins are one maximum)."""
    angles = _paired_angles()
    g = dem("A")
    m = sl.Matcher(g, ctx=gpu_ctx)
    off32 = 0
    for family, params in EXACT.items():
        arr, bbox = described(m, family, params, angles)
        n_twin = m.end_twins(arr, len(params), angles)
        assert n_twin == len(params)
        ids = (np.repeat(np.asarray(params, float), len(angles)), np.tile(angles, len(params)))
        for Tx in FAST_TX:
            sp = sl._lib.sc_plan(**forced_plan(m.ny, m.nx, bbox, Ty, Tx, group=len(params)))
            assert m.can_flag_near_ties(arr, sp)
            st = m.run_described(arr, sp, m.exact_window_for(arr, sp), n_twin)
            chk = check(gpu_ctx.get_result(*ids), "A", family, params, angles)
            m.run_described(arr, sp)
            chk32 = check(gpu_ctx.get_result(*ids), "A", family, params, angles)
            print("exact %s Ty=%d Tx=%d: n_inexact=%d n_bad=%d (float32 mode: n_inexact=%d n_bad=%d) %s"
                  % (family, Ty, Tx, chk["n_inexact"], chk["n_bad"], chk32["n_inexact"], chk32["n_bad"], st))
            assert chk["n_inexact"] == 0 and chk["n_bad"] == 0, (family, Ty, Tx, chk["n_inexact"], chk["n_bad"])
            off32 += chk32["n_inexact"]
    # (the float32 search of the same plans is off the argmax somewhere: the count above can fail)
    assert off32 >= 1, off32


def test_slow_row_kernel_and_masks_cannot_flag(gpu_ctx):
    """(c) the predicate the drivers re-plan by: no near-tie flags from k_inv_rows (Tx of 64 .. 256 and 4096) nor under
    per-cell masks - for those plans the library is not called with the near window on."""
    angles = _paired_angles()
    m = sl.Matcher(dem("A"), ctx=gpu_ctx)
    for family, params in list(EXACT.items()) + [("upper", (2.0, 10.0)), ("upper-p0", (2.0, 10.0))]:
        arr, bbox = described(m, family, params, angles)
        for Ty in SIZES:
            for Tx in SIZES:
                sp = sl._lib.sc_plan(**forced_plan(m.ny, m.nx, bbox, Ty, Tx, group=len(params)))
                assert m.can_flag_near_ties(arr, sp) == (Tx in FAST_TX and not family.startswith("upper")), (family, Ty, Tx)


def test_same_bits_twice(gpu_ctx):
    """(d) one plan from the middle of the matrix - generic column path, fast row kernel, a whole tile pair - run twice
    from a fresh record: the same record bit for bit."""
    m = sl.Matcher(dem("A"), ctx=gpu_ctx)
    for family in ("scarp", "upper-p0"):
        arr, bbox = described(m, family)
        sp = sl._lib.sc_plan(**forced_plan(m.ny, m.nx, bbox, 4096, 512, nty=2, group=GROUP))
        recs = []
        for _ in range(2):
            gpu_ctx.reset_best()
            gpu_ctx.match(arr, sp)
            recs.append([a.copy() for a in gpu_ctx.get_best()])
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*recs)), family
