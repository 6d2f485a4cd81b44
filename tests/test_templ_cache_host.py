"""The template cache's key and its book-keeping of budget and LRU (scarplet_amd/csrc/sc_templ_cache.h) on the host.
tests/templ_cache_check.cpp builds the keys of equal and of singly changed chunks, runs seeded access sequences against a
restated LRU list with the device allocations stubbed out, and follows a search larger than the budget.  A program of its
own under AddressSanitizer and UBSan; nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ builds this test's program: it is not on PATH"
    out = str(tmp_path_factory.mktemp("templ_cache") / "templ_cache_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "templ_cache_check.cpp"), "-o", out], check=True)
    return out


def test_keys_budget_and_lru(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"templ_cache_check: (\d+) checks, (\d+) failed", r.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_the_binding_names_the_two_entries():
    from scarplet_amd import _lib
    assert "sc_forget_templates" in _lib.SIGNATURES and "sc_templ_cache_info" in _lib.SIGNATURES
    assert callable(_lib.Context.forget_templates) and callable(_lib.Context.templ_cache_info)
