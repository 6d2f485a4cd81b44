"""Option "fuse_fwd": the wave-per-column pass (k_inv_cols_w8 / k_inv_cols_w4) runs the curvature's forward column
transform on the columns it parks, instead of a k_fwd_cols launch per orientation that writes uc / uc2.

The fused prologue uses the butterflies, twiddle bases and operand order of k_fwd_cols, so everything downstream must
be the same in EVERY BIT with the option on (the default) and off: the float32 record (snr, amp, id), the near-tie
flags of the exact mode and the settled result.  Two searches:

* C2-sized: the 2048 x 2048 synthetic DEM, C2's ten ages, 13 of its 91 orientations - three tiles of 1024 x 2048,
  orientations batched: a tile pair on k_inv_cols_w8<1024, false>, the third tile alone, its templates in pairs, on
  k_inv_cols_w8<1024, true>;
* a reduced C3: the synthetic DEM at 5000 x 5000 = 3 x 3 tiles of 2048, 5 ages x 7 orientations - four tile pairs on
  k_inv_cols_w8<2048, false>, interleaved two per launch, and the ninth tile alone on k_inv_cols_w4<2048, true>.

That the fused form really ran is read from the launch counts: one k_fwd_cols launch less per forward curvature pass.
Kept spectra (option "spectra_mb") are uc / uc2 and switch the fused form off, so the context here keeps none."""
import numpy as np
import pytest

import scarplet_amd as sl
from scarplet_amd import _plan, synthetic

pytestmark = pytest.mark.gpu


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint8)


def _run(ctx, g, ages, angles, fuse, tiles):
    ctx.set_option("fuse_fwd", fuse)
    m = sl.Matcher(g, ctx=ctx)
    ctx.profile(1)
    m.search(sl.Scarp, 100, ages, angles, method="fft")
    prof = ctx.profile_get()
    ctx.profile(0)
    p = m.plan
    assert (p.Ty, p.Tx, p.nty, p.ntx) == tiles, p
    out = {"f32 %s" % k: np.array(v) for k, v in zip(("amp", "snr", "id"), ctx.get_best())}
    for k, v in zip(("amp", "age", "angle", "snr"), m.result()):
        out["f32 result %s" % k] = np.array(v)
    m.search(sl.Scarp, 100, ages, angles, method="fft", exact=True)
    assert m.method_used == "fft", m.method_used
    out["near-tie flags"] = np.array(ctx.near_ties())
    for k, v in zip(("amp", "age", "angle", "snr"), m.result()):
        out["exact result %s" % k] = np.array(v)
    return out, {k: prof[k][0] for k in ("k_fwd_rows", "k_fwd_cols", "k_inv_cols")}, dict(m.exact_stats)


@pytest.mark.parametrize("case", ["C2-sized", "reduced C3"])
def test_fused_forward_changes_no_bit(case):
    ages35 = _plan.age_grid()
    if case == "C2-sized":
        n, tiles = 2048, (1024, 2048, 3, 1)
        ages = ages35[np.round(np.linspace(0, 34, 10)).astype(int)]
        angles = _plan.angle_grid(-np.pi / 4, np.pi / 4)[::7]                    # 13 of C2's 91
    else:
        n, tiles = 5000, (2048, 2048, 3, 3)
        ages = ages35[np.round(np.linspace(0, 34, 5)).astype(int)]
        angles = _plan.angle_grid()[[0, 23, 45, 90, 135, 157, 180]]
    g = synthetic.synthetic_scarp(n)
    ctx = sl._lib.Context(0)
    try:
        ctx.set_option("spectra_mb", 0)
        two, n_two, _ = _run(ctx, g, ages, angles, 0, tiles)
        one, n_one, st_one = _run(ctx, g, ages, angles, 1, tiles)
    finally:
        ctx.close()
    print("%s: launches two-launch form %s, fused %s; near-tie cells %d; exact %s"
          % (case, n_two, n_one, int(one["near-tie flags"].sum()), st_one))
    # the fused form ran: the template passes' column launches stay (k_fwd_cols_tsym has the same slot), the
    # curvature's are gone - one per forward curvature pass
    assert n_one["k_fwd_rows"] == n_two["k_fwd_rows"] and n_one["k_inv_cols"] == n_two["k_inv_cols"], (n_one, n_two)
    assert 0 < n_two["k_fwd_cols"] - n_one["k_fwd_cols"] <= len(angles), (n_one, n_two)
    assert int(one["near-tie flags"].sum()) > 0                                 # (the exact mode had something to settle)
    assert sorted(one) == sorted(two)
    for k in sorted(one):
        a, b = one[k], two[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        diff = int(np.count_nonzero(_bits(a) != _bits(b)))
        assert diff == 0, "%s: %s differs in %d bytes" % (case, k, diff)
