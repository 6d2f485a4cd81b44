"""The adversarial trace layouts (tests/trace_shapes.py) on the host: what the numpy reference makes of them.  These
are the conditions that keep tests/test_gpu_trace_shapes.py from being vacuous - each curve really is one component
far longer than a scan block, a radix block and a wave, and the diagonals really are separate."""
import numpy as np
import pytest
from scipy import ndimage

import trace_reference as tr
import trace_shapes as ts

# cells of the mask as drawn (the generators are the specification of the shapes)
CELLS = {"checkerboard_200": 20000, "serpentine_200_p2": 20099, "serpentine_97x131_p3": 4387, "comb_130x200": 13100,
         "diagonals_150": 5626, "spiral_201": 10396}
ONE_CURVE = [n for n in ts.SMALL if n != "diagonals_150"]


@pytest.mark.parametrize("name", list(ts.SMALL))
def test_cell_counts_and_sectors(name):
    mask, sector = ts.shape(name)
    assert mask.dtype == bool and int(mask.sum()) == CELLS[name]
    p = ts.planes_of(mask, sector, 0)
    assert p.shape == (4,) + mask.shape and p.dtype == np.float64
    assert np.array_equal(tr.sectors(p[2]), sector)
    assert np.array_equal(p[3] > 0, mask) and p[3][mask].min() >= 3.0 and p[3][mask].max() < 4.0


@pytest.mark.parametrize("name, variant", [(n, v) for n in ONE_CURVE for v in ts.variants(n)])
def test_one_curve_is_one_segment(name, variant):
    mask, p = ts.planes(name, variant)
    thin, labels, tab = tr.trace(p, *ts.SETTINGS)
    assert not (thin & ~mask).any()
    assert len(tab["first"]) == 1
    assert tab["n_cells"][0] >= 0.95 * mask.sum()
    assert tab["n_cells"][0] > 4096                                    # one scan block, one radix block
    assert tab["n_cells"][0] == thin.sum() == (labels == 1).sum()


def test_checkerboard_is_thin_as_drawn():
    mask, p = ts.planes("checkerboard_200")
    thin, _, tab = tr.trace(p, *ts.SETTINGS)
    assert np.array_equal(thin, mask) and tab["n_cells"][0] == 20000


@pytest.mark.parametrize("variant", ["plain", "flipped"])
def test_diagonals_stay_apart(variant):
    mask, p = ts.planes("diagonals_150", variant)
    thin, labels, tab = tr.trace(p, *ts.SETTINGS)
    assert np.array_equal(thin, mask)
    comp, nc = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
    assert nc == 75 and len(tab["first"]) == 75                        # every diagonal has a strong cell at this seed
    assert np.array_equal(labels > 0, mask)
    # the same partition: one label per scipy component and the reverse
    pairs = np.unique(np.stack([comp[mask], labels[mask]]), axis=1)
    assert pairs.shape[1] == 75
    assert tab["n_cells"].max() == 150 > 64 and tab["n_cells"].sum() == 5626
    assert np.array_equal(np.sort(tab["n_cells"]), np.sort(np.bincount(comp[mask])[1:]))


def test_the_large_serpentine():
    mask, sector = ts.serpentine(1024, 1024, 2)
    assert mask.sum() == 524799
    _, _, tab = tr.trace(ts.planes_of(mask, sector, 7), *ts.SETTINGS)
    assert len(tab["first"]) == 1 and tab["n_cells"][0] >= 0.95 * 524799


def test_transpose_and_flip_are_involutions():
    for name in ts.SMALL:
        mask, sector = ts.shape(name)
        for f in (ts.transpose, ts.fliplr):
            m2, s2 = f(*f(mask, sector))
            assert np.array_equal(m2, mask) and np.array_equal(s2, sector)
