"""The C-ABI library loads and exports everything include/scarplet_hip.h
declares; struct layouts seen by ctypes equal the C compiler's.  No compute
calls (there is no GPU on the CPU test box)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from scarplet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scarplet_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "missing export: " + n
    assert sorted(_lib.SIGNATURES) == names, "ctypes table out of sync with the header"


C_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64,
             "size_t": ctypes.c_size_t}
C_POINTEES = {"double": ctypes.c_double, "float": ctypes.c_float, "int": ctypes.c_int, "int32_t": ctypes.c_int32,
              "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "long long": ctypes.c_longlong,
              "unsigned long long": ctypes.c_ulonglong, "char": ctypes.c_char}


def header_prototypes():
    """{name: (return type, [parameter types])} of include/scarplet_hip.h, the types as C spells them less ``const`` and
    the parameter's name.  The prototypes are regular: ``int sc_x(type name, ...);``."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)

    def ctype(text, named):
        toks = [t for t in text.replace("*", " * ").split() if t != "const"]
        if named and toks != ["void"]:
            toks = toks[:-1]                                # the parameter's name
        return " ".join(toks).replace(" *", "*")
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(sc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        assert name not in out, name
        params = [ctype(p, True) for p in params.split(",")]
        out[name] = (ctype(ret, False), [] if params == ["void"] else params)
    return out


def check_type(c, t, where):
    """The C type ``c`` against the ctypes type ``t`` of the table."""
    if not c.endswith("*"):
        want = None if c == "void" else C_SCALARS[c]
        assert t is want, "%s: %s in the header, %r in the table" % (where, c, t)
        return
    pointer = isinstance(t, type) and issubclass(t, ctypes._Pointer)
    assert t in (ctypes.c_void_p, ctypes.c_char_p) or pointer, "%s: %s in the header, %r in the table" % (where, c, t)
    if pointer:
        pointee = c[:-1].strip()
        want = ctypes.c_void_p if pointee.endswith("*") else C_POINTEES.get(pointee) or getattr(_lib, pointee)
        assert t._type_ is want, "%s: %s in the header, a pointer to %r in the table" % (where, c, t._type_)
    if t is ctypes.c_char_p:
        assert c == "char*", "%s: %s in the header, c_char_p in the table" % (where, c)


def test_every_prototype_of_the_header_has_its_types_in_the_table():
    """Every prototype of include/scarplet_hip.h against its SIGNATURES entry: the number of parameters, each scalar's
    type, a pointer-like type for each pointer and, where the table names a pointee, the C pointee.  ctypes itself takes
    a wrong type or a wrong order without complaint."""
    protos = header_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES) == declared_functions()
    for name, (ret, params) in protos.items():
        res, args = _lib.SIGNATURES[name]
        check_type(ret, res, name + " returns")
        assert len(params) == len(args), "%s: %d parameters in the header, %d in the table" % (name, len(params), len(args))
        for i, (c, t) in enumerate(zip(params, args)):
            check_type(c, t, "%s, parameter %d" % (name, i))


def test_host_library_exports_every_declared_symbol():
    """libscarplet_host.so (include/scarplet_host.h): plain C, linked against nothing of ROCm."""
    from scarplet_amd import _hostlib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scarplet_host.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(sch_[a-z0-9_]+)\s*\(", src)))
    lib = ctypes.CDLL(_hostlib.LIB_PATH)
    assert names and sorted(_hostlib.SIGNATURES) == names
    for n in names:
        assert hasattr(lib, n), "missing export: " + n
    needed = subprocess.check_output(["readelf", "-d", _hostlib.LIB_PATH]).decode()
    assert "amdhip" not in needed and "rccl" not in needed


def test_load_binds_and_reports_version():
    lib = _lib.load()
    assert lib.sc_abi_version() == _lib.ABI_VERSION
    assert lib.sc_kernel_name(_lib.K_INV_ROWS) == b"k_inv_rows"


def test_struct_layouts_match_c(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "scarplet_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(sc_template), offsetof(sc_template, cc),
         offsetof(sc_template, ilo), offsetof(sc_template, id), sizeof(sc_plan), sizeof(sc_xfer));
  return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T = _lib.sc_template
    assert vals == [ctypes.sizeof(T), T.cc.offset, T.ilo.offset, T.id.offset,
                    ctypes.sizeof(_lib.sc_plan), ctypes.sizeof(_lib.sc_xfer)]


def test_product_fails_loudly_without_gpu():
    if os.path.exists("/dev/kfd"):          # no HIP call here: later tests start subprocesses
        pytest.skip("a GPU box")
    lib = _lib.load()
    if lib.sc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.ScarpletHipError):
        _lib.Context(0)
    import numpy as np
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((32, 32)), 1.0)
    with pytest.raises(_lib.ScarpletHipError):
        sl.match(g, sl.Scarp, scale=5, age=10.)


def test_product_does_not_import_the_oracle():
    code = ("import sys; import scarplet_amd, scarplet_amd.dist, scarplet_amd.synthetic; "
            "assert not [m for m in sys.modules if 'oracle' in m], 'oracle imported'")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "scarplet_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                assert "scarplet_oracle" not in open(os.path.join(dirpath, f)).read(), f
