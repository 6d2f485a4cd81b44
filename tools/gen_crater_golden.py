#!/opt/conda/bin/python3.9
"""Golden fixture of the reference's Crater.template() (WindowedTemplate.py:528-605).

Runs where the reference and the Anaconda interpreter are (like oracle/gen_golden.py, whose
import_reference() it uses):

    /opt/conda/bin/python3.9 tools/gen_crater_golden.py

Calls the UNMODIFIED reference class for six (r, kt, nx, ny, de) and writes tests/golden/ref_crater.npz in
the layout of conftest.load_cases: the inputs and the (ny, nx) float64 template of every case.  Odd and even
grids, rectangular grids, de != 1, a ring of three cells and one of forty.

It also checks what makes "the same support, cell for cell" a fair demand on a restatement: no non-zero
reference cell lies below 1e-9 of the template's largest - the support is decided by the two mask compares,
never by what a cancellation between strips of opposite sign leaves behind.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import import_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# (r, kt, nx, ny, de)
CASES = [(10, 1, 64, 64, 1), (10, 10, 65, 63, 1), (20, 3, 96, 80, 2), (6, 0.5, 33, 33, 1), (3, 1, 32, 32, 1),
         (40, 30, 128, 128, 1)]
RESIDUE = 1e-9


def main():
    _, _, WT = import_reference()
    out = {"n": np.array(len(CASES))}
    for i, (r, kt, nx, ny, de) in enumerate(CASES):
        W = np.asarray(WT.Crater(r, kt, nx, ny, de).template(), dtype=np.float64)
        assert W.shape == (ny, nx) and np.isfinite(W).all()
        nz = np.abs(W[W != 0])
        assert nz.size and nz.min() >= RESIDUE * nz.max(), (i, nz.min(), nz.max())
        print("case %d: r %g kt %g %d x %d de %g: %d non-zero cells, max|W| %.6g, smallest / largest %.3g"
              % (i, r, kt, ny, nx, de, nz.size, nz.max(), nz.min() / nz.max()), flush=True)
        for k, v in (("r", float(r)), ("kt", float(kt)), ("nx", nx), ("ny", ny), ("de", float(de)), ("W", W)):
            out["%s_%d" % (k, i)] = np.asarray(v)
    np.savez_compressed(os.path.join(GOLDEN, "ref_crater.npz"), **out)
    print("wrote tests/golden/ref_crater.npz")


if __name__ == "__main__":
    main()
