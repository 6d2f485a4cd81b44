"""Host side of exact=True for host-uploaded windows, without a device: the settle's audit as the Python layer decodes it,
the orientation-sharded settle's refusal of window templates, and the ABI version of the header and the binding."""
import ctypes
import os
import re

import pytest

from scarplet_amd import _lib
from scarplet_amd import WindowedTemplate as WT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_settle_stats_decode_the_audit():
    st = (ctypes.c_longlong * 8)(5, 9, 7, 4, 2, 30, 123456, 800)
    d = _lib.Context._settle_stats(st)
    assert d["max_f32_err"] == pytest.approx(1.23456e-4, rel=1e-12)
    assert (d["flagged_cells"], d["pairs_listed"], d["float64_pairs"], d["float64_cells"], d["changed_cells"],
            d["events"], d["taps"]) == (5, 9, 7, 4, 2, 30, 800)
    assert _lib.Context._settle_stats((ctypes.c_longlong * 8)())["max_f32_err"] == 0.0


class _NoCallLib(object):
    """A library that must not be reached."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


class _FakeContext(object):
    lib = _NoCallLib()
    _h = None
    _exchanged = 0
    _settle_stats = staticmethod(_lib.Context._settle_stats)


def _templates(kinds):
    arr = (_lib.sc_template * len(kinds))()
    for k, kind in enumerate(kinds):
        arr[k].kind = kind
        arr[k].id = k
        arr[k].window = 0 if kind == WT.KIND_WINDOW else -1
    return arr


def test_settle_pairs_refuses_window_templates():
    arr = _templates([WT.KIND_SCARP, WT.KIND_WINDOW, WT.KIND_WINDOW])
    with pytest.raises(_lib.ScarpletHipError, match="host-uploaded windows"):
        _lib.Context.settle_pairs(_FakeContext(), arr, None)


def test_settle_pairs_passes_builtin_templates_to_the_library():
    calls = []

    class Lib(object):
        def sc_settle_pairs(self, *a):
            calls.append(a)
            return 0

    ctx = _FakeContext()
    ctx.lib = Lib()
    ctx._check = lambda rc, what: None
    st = _lib.Context.settle_pairs(ctx, _templates([WT.KIND_SCARP, WT.KIND_RICKER]), None)
    assert len(calls) == 1 and st["max_f32_err"] == 0.0


def test_library_refuses_window_templates_in_settle_pairs():
    """The library itself says so too (the check sits in sc_settle_pairs, before the template table is loaded)."""
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_settle.hip")).read()
    body = src[src.index('extern "C" int sc_settle_pairs'):]
    body = body[:body.index("sc_load_templates")]
    assert "SC_KIND_WINDOW" in body and "SC_ERR_UNSUPPORTED" in body


def test_header_abi_version_is_the_bindings():
    src = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    v = int(re.search(r"#define\s+SC_ABI_VERSION\s+(\d+)", src).group(1))
    assert v == _lib.ABI_VERSION == 10
