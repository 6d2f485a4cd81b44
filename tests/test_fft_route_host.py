"""The FFT path's route (scarplet_amd/csrc/sc_fft_route.h) on the host: tests/fft_route_check.cpp enumerates its inputs -
every tile size pair, parities, tile counts, masks, maps, near-tie flags, batches, kept spectra, the "variant" options - and
asserts invariants: kernels named only at the sizes they are instantiated for, the near-tie refusal exactly where
Matcher.can_flag_near_ties says no, the shapes DESIGN.md names.  A program of its own under AddressSanitizer and UBSan;
nothing is loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_route_invariants(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ builds this test's program: it is not on PATH"
    exe = str(tmp_path / "fft_route_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "fft_route_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout, r.stdout
