#!/usr/bin/env python3
"""Developer check: what the Python binding of the fit family hands to the library, as text - the whole SIGNATURES table,
the structured dtypes of the rows, and the (name, arguments) log of every wrapper in every form through a recording fake
library (tests/test_fit_binding_host.py: no device).  Two trees whose bindings agree print the same lines: run it once per
tree (--package DIR takes scarplet_amd from another checkout) and diff.  The dtypes are printed field by field;
their reprs come last, under a heading of their own, since numpy marks a dtype it derived from a ctypes Structure
``align=True`` where the layout is the same."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--package", default=ROOT, help="the checkout whose scarplet_amd is described")
a = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(a.package))


def tname(t):
    return "None" if t is None else t.__name__


def main():
    import test_fit_binding_host as fb
    from scarplet_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))) == os.path.abspath(a.package)
    print("# signatures")
    for name, (res, args) in _lib.SIGNATURES.items():
        print("%s: %s (%s)" % (name, tname(res), ", ".join(tname(t) for t in args)))
    dtypes = sorted(k for k in vars(_lib) if k.endswith("_DTYPE"))
    print("# dtypes: %d" % len(dtypes))
    for k in dtypes:
        d = getattr(_lib, k)
        print("%s: itemsize %d, %s" % (k, d.itemsize, ", ".join("%s %s @%d" % (f, d.fields[f][0].str, d.fields[f][1])
                                                                 for f in d.names)))
    print("# calls")
    for line in fb.replay():
        print(line)
    print("# dtype reprs")
    for k in dtypes:
        print("%s: %r" % (k, getattr(_lib, k)))


if __name__ == "__main__":
    main()
