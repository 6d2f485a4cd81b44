"""Adversarial layouts for the traces of a result (docs/traces.md): one-cell-wide curves that the thinning rule keeps as
drawn, so that the labelling (union-find per 32 x 32 tile, merges across tile borders, flatten), the scans, the radix
sort and the per-segment reduction see what random planes never give them - one component through every tile, long
parent chains, thousands of merges on one root, a segment far longer than a scan or radix block.  Not a test module.

Every generator returns (mask bool, sector int 0..3).  A cell is thin when its two neighbours along its own sector's
step (trace_reference.STEPS) are lower, so a curve whose cells carry a sector that steps ACROSS the curve, with
snr > 0 on it and 0 off it, survives thinning (but for a few junction cells, where two arms touch)."""
import numpy as np


def checkerboard(ny, nx):
    """Every second cell, all sector 0 (step along the row, onto empty cells): diagonal links only, inside the tiles and
    across every tile border and corner.  thin == mask exactly; one component."""
    r, c = np.indices((ny, nx))
    return (r + c) % 2 == 0, np.zeros((ny, nx), dtype=np.int64)


def serpentine(ny, nx, pitch=2):
    """Rows 0, pitch, 2 pitch, ... in sector 2 (step down the column), joined alternately at the last and the first
    column by sector-0 cells: one path through every tile."""
    mask = np.zeros((ny, nx), dtype=bool)
    sector = np.zeros((ny, nx), dtype=np.int64)
    rows = np.arange(0, ny, pitch)
    mask[rows] = True
    sector[rows] = 2
    for k, r in enumerate(rows[:-1]):
        c = nx - 1 if k % 2 == 0 else 0
        mask[r + 1:r + pitch, c] = True                                # (sector 0 already)
    return mask, sector


def comb(ny, nx):
    """Row 0 in sector 2 and every second column below it in sector 0: teeth that meet only in row 0."""
    mask = np.zeros((ny, nx), dtype=bool)
    sector = np.zeros((ny, nx), dtype=np.int64)
    mask[1:, 0::2] = True
    mask[0] = True
    sector[0] = 2
    return mask, sector


def diagonals(ny, nx):
    """The diagonals (r - c) % 4 == 0 in sector 1 (step along the anti-diagonal): parallel segments that must NOT
    merge, each crossing tile corners."""
    r, c = np.indices((ny, nx))
    return (r - c) % 4 == 0, np.ones((ny, nx), dtype=np.int64)


def spiral(n):
    """A rectangular spiral of pitch 4 from the corner (0, 0) inwards: horizontal arms in sector 2, vertical arms in
    sector 0 (the corner cells belong to the horizontal arms)."""
    mask = np.zeros((n, n), dtype=bool)
    sector = np.zeros((n, n), dtype=np.int64)
    k = 0
    while n - 1 - 8 * k >= 4:
        lo, hi = 4 * k, n - 1 - 4 * k
        mask[lo, max(lo - 4, 0):hi + 1] = True                         # top arm, from the end of the last ring
        sector[lo, max(lo - 4, 0):hi + 1] = 2
        mask[hi, lo:hi + 1] = True                                     # bottom arm
        sector[hi, lo:hi + 1] = 2
        mask[lo + 1:hi, hi] = True                                     # right arm
        mask[lo + 5:hi, lo] = True                                     # left arm, up to the next ring's top arm
        k += 1
    return mask, sector


def transpose(mask, sector):
    """The shape mirrored at the main diagonal: sectors 0 and 2 change places, 1 and 3 keep theirs."""
    s = sector.T.copy()
    s[sector.T == 0] = 2
    s[sector.T == 2] = 0
    return np.ascontiguousarray(mask.T), s


def fliplr(mask, sector):
    """The shape mirrored left to right: sectors 1 and 3 change places."""
    f = sector[:, ::-1]
    s = f.copy()
    s[f == 1] = 3
    s[f == 3] = 1
    return np.ascontiguousarray(mask[:, ::-1]), s


def planes_of(mask, sector, seed, snr_const=None):
    """(amp, age, angle, snr) as one (4, ny, nx) float64 array: snr 3 + U[0, 1) on the mask (or the one constant
    ``snr_const``) and 0 elsewhere, angles 0, pi/4, pi/2, 3 pi/4 for the sectors 0 to 3."""
    rng = np.random.default_rng(seed)
    u = rng.random(mask.shape)
    snr = np.where(mask, 3.0 + u if snr_const is None else float(snr_const), 0.0)
    ang = sector * (np.pi / 4)
    amp = rng.standard_normal(mask.shape)
    age = 10 ** rng.uniform(0, 3.5, mask.shape)
    return np.stack([amp, age, ang, snr])


# name -> (generator, arguments, seed of planes_of): the shapes that the host test pins and the device test runs
SMALL = {
    "checkerboard_200": (checkerboard, (200, 200), 1),
    "serpentine_200_p2": (serpentine, (200, 200, 2), 2),
    "serpentine_97x131_p3": (serpentine, (97, 131, 3), 3),
    "comb_130x200": (comb, (130, 200), 4),
    "diagonals_150": (diagonals, (150, 150), 7),
    "spiral_201": (spiral, (201,), 6),
}
GIANTS = ("checkerboard_200", "serpentine_200_p2", "comb_130x200", "spiral_201")       # largest segment > 4096 cells
TRANSPOSABLE = ("serpentine_200_p2", "serpentine_97x131_p3", "comb_130x200")
SETTINGS = (1.0, 3.5, 1)                                               # snr_low, snr_high, min_cells


def variants(name):
    """plain, flipped, and transposed where the transpose is another shape (chains that run down the columns)."""
    return ("plain", "transposed", "flipped") if name in TRANSPOSABLE else ("plain", "flipped")


def shape(name):
    gen, args, _ = SMALL[name]
    return gen(*args)


def planes(name, variant="plain", snr_const=None):
    """The planes of a named shape; ``variant``: plain, transposed or flipped."""
    mask, sector = shape(name)
    if variant == "transposed":
        mask, sector = transpose(mask, sector)
    elif variant == "flipped":
        mask, sector = fliplr(mask, sector)
    return mask, planes_of(mask, sector, SMALL[name][2], snr_const)
