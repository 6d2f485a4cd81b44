"""The checker of tests/test_gpu_direct_classes.py has teeth on every probe window (CPU only).

The oracle's own fold of a window's stack - the result a perfect device returns - passes check_window with nothing
bad and nothing off the argmax.  The same fold shifted by one column (an indexing slip at a seam), and the same fold
labelled with the next template's (age, angle) (a slip in the template loop), must both come back with n_bad > 0 on
every window the GPU test probes.  A window on which they do not is one where every template is masked - the corners
and the last patches under the Scarp family's window limits, a window on the far side of every UpperBreak template's
error half-plane - where the zero record is all there is to check; each such window must be live (all templates
unmasked) in a Ricker case of the same DEM, where the shifted folds are caught."""
import numpy as np
import pytest

import direct_classes as dc


@pytest.fixture(scope="module")
def pool():
    import multiprocessing as mp
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    p = mp.get_context("fork").Pool(max(1, min(n, 8)))
    yield p
    p.terminate()
    p.join()


def probes(res, c):
    """The fold shifted by one column, and labelled with the next template."""
    amp, age, ang, snr = res
    shifted = tuple(np.roll(a, 1, axis=1) for a in res)
    p_of, a_of = dc.ids(c)
    T = len(p_of)
    nxt = np.zeros(amp.shape, dtype=np.int64)
    for t in range(T):
        nxt[(age == p_of[t]) & (ang == a_of[t]) & (snr > 0)] = (t + 1) % T
    live = snr > 0
    relabelled = (amp, np.where(live, p_of[nxt], 0.0), np.where(live, a_of[nxt], 0.0), snr)
    return shifted, relabelled


def test_checker_has_teeth_on_every_probe_window(pool):
    seen, dead, ricker_live = set(), [], set()
    n_windows = 0
    for c in dc.CASES:
        key = (c["dem"], c["family"], c["scale"], c["params"], c["angles"])
        if key in seen:
            continue
        seen.add(key)
        for (label, win, live, a_st, s_st) in dc.oracle_windows(c, pool):
            res = dc.oracle_fold(a_st, s_st, c)
            chk = dc.check_window(res, c, a_st, s_st)
            assert chk["n_bad"] == 0 and chk["n_inexact"] == 0, (c["name"], label)
            if s_st.max() == 0:
                assert c["family"] != "ricker", (c["name"], label)
                dead.append((c["dem"], win, c["name"], label))
                continue
            if live and c["family"] == "ricker":
                ricker_live.add((c["dem"], win))
            for what, bad in zip(("one column", "one template"), probes(res, c)):
                n_bad = dc.check_window(bad, c, a_st, s_st)["n_bad"]
                assert n_bad > 0, (c["name"], label, win, what)
            n_windows += 1
    # windows where every template of a Scarp-family case is masked: the same cells are probed, live, by a Ricker case
    for (name, win, case, label) in dead:
        assert (name, win) in ricker_live, (case, label, win)
    assert n_windows > 200 and len(dead) > 0


def float32_chain_error(z, W, angle):
    """The largest relative SNR error, over the DEM's cells, of xcorr and T3 accumulated as plain float32 chains over the
    window's taps (one fused multiply-add per tap, as the kernel's) against the same sums in float64 - the number
    format's error for this window on this DEM, by check_fold's measure (relative to the cell's SNR, cells below a
    thousandth of the map's maximum to that floor)."""
    import scarplet_oracle as orc
    c64 = orc.directional_curvature(z, 1.0, 1.0, angle).astype(np.float32).astype(np.float64)
    ks, ls = np.nonzero(W)
    w = W[ks, ls].astype(np.float32).astype(np.float64)
    xc, t3 = np.zeros(c64.shape, np.float32), np.zeros(c64.shape, np.float32)
    xc64, t364 = np.zeros(c64.shape), np.zeros(c64.shape)
    for k, l, wk in zip(ks, ls, w):
        v = np.roll(np.roll(c64, k - W.shape[0] // 2, 0), l - W.shape[1] // 2, 1)
        xc = (xc.astype(np.float64) + wk * v).astype(np.float32)            # (a product of two float32 is exact in float64)
        t3 = (t3.astype(np.float64) + v * v).astype(np.float32)
        xc64 += wk * v
        t364 += v * v
    ts, n = float(np.sum(w ** 2)), len(w)

    def snr(x, t):
        amp = x / ts
        T1 = ts * amp * amp
        return np.abs(T1 / ((T1 - 2 * amp * x + t) / n + orc.EPS))
    s32, s64 = snr(xc.astype(np.float64), t3.astype(np.float64)), snr(xc64, t364)
    return float(np.max(np.abs(s32 - s64) / np.maximum(s64, 1e-3 * s64.max())))


def test_uploaded_windows_are_within_a_float32_chain_s_reach():
    """The uploaded windows of the GPU test are about rows, runs and slabs, not about how many taps a float32 sum bears:
    on the small DEM a plain float32 chain over each window's taps stays below 4e-5, four fifths of what report() allows
    the device (half the real-space tie window).  The first form of the tall window - 3045 taps around a constant 2.0 -
    is at 8.6e-5 by the same measure (the device: 9.1e-5): kept here as the counter-example."""
    import scarplet_oracle as orc
    z = np.asarray(dc.dem("S")._griddata, dtype=float)
    half = 0.5 * orc.tie_window("direct")
    for name, W in (("tall 142", dc.tall_window(142)), ("runs", dc.run_length_window())):
        e = float32_chain_error(z, W, 0.4)
        print("float32 chain, %s (%d taps) on S: %.2e" % (name, np.count_nonzero(W), e))
        assert e <= 0.8 * half, (name, e)
    a, b = np.arange(161)[:, None], np.arange(21)[None, :]
    dense = np.sin(0.21 * a + 0.5 * b) + 0.4 * np.cos(0.05 * a * b) + 2.0
    assert float32_chain_error(z, dense, 0.4) > half
