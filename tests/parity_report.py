"""report(): the line every fold check of the GPU suite prints, and the policy it asserts (shared by the test modules)."""
import scarplet_oracle as orc


def report(name, chk, method="fft", window=None, noise_floor=True, max_inexact=0):
    """One line per fold check in the test log (pytest -s / GPUTEST output), and the two policies:
    the SNR error this check measured is at most half the tie window of the device path that
    ran ('auto' searches are judged by the wider FFT window); and the argmax is EXACT as an
    integer - `inexact` = cells with a decidable argmax (above the absolute SNR tolerance) that
    do not carry the oracle's own (age, angle) - which must be 0 on every DEM with a noise floor
    of its own (lidar, the benchmark DEM, every synthetic DEM with sigma > 0).  Cells below the
    absolute tolerance on both sides are reported as `below`, not counted as exact.  Only the
    surfaces WITHOUT a noise floor (noise_floor=False: test_noise_free_surfaces_resolution_floor
    and the like) are held to a fraction, EXACT_MIN.  max_inexact: the two checks of the suite
    that are NOT exact on the FFT path say so with their measured count (a handful of cells in
    several hundred thousand whose two best templates lie closer together, in the oracle's own
    float64 SNRs, than the float32 FFT convolution's measured error on that DEM - `gap` in the
    line); the real-space path is exact on the same inputs."""
    # (the window the check itself ran with - per path AND per template family, oracle.tie_window)
    window = chk.get("tie_rtol", orc.tie_window(method)) if window is None else window
    print("fold %-44s bad=%d inexact=%d (gap %.1e) below=%d exact=%.6f strict=%d tie=%d of %d snr_err=%.2e amp_err=%.2e (window %.0e)"
          % (name, chk["n_bad"], chk["n_inexact"], chk["inexact_gap"], chk["n_below_only"], chk["exact_frac"], chk["n_strict"],
             chk["n_tie"], chk["n"], chk["snr_err"], chk["amp_err"], window))
    assert chk["snr_err"] <= 0.5 * window, (name, chk["snr_err"], window)
    if noise_floor:
        assert chk["n_inexact"] <= max_inexact, (name, "cells off the oracle's argmax:", chk["n_inexact"], "of", chk["n"])
        # ... and those that are allowed lie inside the tie window (twice the largest error measured on the path)
        assert chk["inexact_gap"] <= window, (name, chk["inexact_gap"], window)
    # (noise_floor=False: the caller states what it expects of exact_frac - EXACT_MIN on the exact
    #  real-space path, the measured 0.90 .. 0.99 of the FFT path inside its per-cell resolution)
