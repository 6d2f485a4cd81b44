"""The case table of the real-space path's kernel classes (test infrastructure, no device access).

launch_direct asks direct_route (scarplet_amd/csrc/sc_direct_route.h) which of the eight instantiations
k_direct2<NB, RW, SHARE, W4> a launch takes: by the core's extent (how many workgroups a patch of 512 x 16, 256 x 16 or
256 x 8 cells gives), by the launch's largest window box (does its slab fit half the LDS - the W4 class - or the 512
patch at all), by whether some template of the orientation run has hole-free rows of SC_DR_SHARE_MIN taps (SHARE) and by
the option "variant" (11: SHARE off, 16: no 512 patch, 19: no W4).  match_impl decides how many orientations ride in one
launch (direct_batch_want), the kernel in how many slabs a template is staged (direct_slab_rows).

Every case below NAMES what it reaches: its classes, whether its orientations are batched, whether some template is
staged in several slabs, whether the DEM is narrower than the slab (the per-cell wrap of the slab fill).
tests/test_direct_route_host.py asks the route's own functions (tests/direct_route_check.cpp, a host program) and holds
every case to its claim on the CPU; tests/test_gpu_direct_classes.py runs the cases against the float64 oracle.

The window boxes are those of the descriptors (WindowedTemplate.grid_descriptors: what Matcher.describe fills the
sc_template array from); the orientation runs and their chunks are laid out here as match_impl does for searches of at
most 32 orientations whose runs are compatible (the same parity and mask kind: one family per search)."""
import numpy as np

from scarplet_amd import WindowedTemplate as WT

# name -> (ny, nx, seed): synthetic.synthetic_scarp(nx, seed=seed, ny=ny), default noise.  Every DEM has an odd extent
# and none is a multiple of a patch (256 or 512 columns, 8 or 16 rows).
DEMS = {
    "A": (150, 131, 11),          # <1,1>: 10 x 1 patches of 256 x 16 (the DEMs of tests/test_gpu_tile_classes.py), narrower than a slab
    "B": (151, 130, 12),
    "S": (300, 301, 13),          # <1,1>, two patch columns: the uploaded windows
    "M": (1030, 1031, 14),        # 5 x 65 = 325 patches of 256 x 16, 5 x 129 = 645 of 256 x 8: <1,2> / W4, batched
    "N": (4091, 200, 15),         # 1 x 256 patches of 256 x 16: the same, one patch column narrower than its slab
    "U": (1500, 1501, 16),        # 6 x 188 = 1128 patches of 256 x 8: <1,2> / W4, one orientation per launch
    "L": (2050, 2061, 17),        # 5 x 129 = 645 patches of 512 x 16: <2,2>
    "V": (8201, 500, 18),         # 1 x 513 patches of 512 x 16: <2,2>, one (partial) patch column narrower than its slab
}

H = np.pi / 2
# name -> (class, oracle kind)
FAMILIES = {"scarp": (WT.Scarp, "scarp"), "ricker": (WT.Ricker, "ricker"), "upper": (WT.LeftFacingUpperBreakScarp, "left_upper_break")}

C11S, C11 = (1, 1, True, False), (1, 1, False, False)
C12S, C12 = (1, 2, True, False), (1, 2, False, False)
C22S, C22 = (2, 2, True, False), (2, 2, False, False)
W4S, W4 = (1, 2, True, True), (1, 2, False, True)
ALL_CLASSES = {C11S, C11, C12S, C12, C22S, C22, W4S, W4}

ANG = (-H, -0.7, 0.0, 0.9, H)           # 0 and +-pi/2: the Scarp window's hole at xr = 0 (rows without the shared form)
OBL = (-1.1, -0.4, 0.6, 1.2)

# Scarp windows: half width c = 2.33 sqrt(age) across the strike, d = scale along it.
#   thin:  scale 6, ages <= 5: no hole-free row of 16 taps at any angle (2 d = 12, 2 c <= 10.4)
#   small: scale 12, ages <= 50: boxes up to 41 x 41 - (256 + 44) (16 + 40) floats fit half the LDS
#   medium: scale 18, ages <= 100: boxes up to 60 x 60 - not W4, one slab of the 256 x 16 patch's whole LDS
#   large: scale 30, ages <= 300: boxes of 100 rows - two slabs of either 16-row patch
#   tall:  scale 60 at oblique angles, ages <= 1000: 187 rows of 192 taps, 42 rows of the 512 patch's slab at a time
THIN, SMALL, LARGE, TALL = (6, (1.0, 2.0, 5.0)), (12, (2.0, 10.0, 50.0)), (30, (10.0, 100.0, 300.0)), (60, (100.0, 1000.0))
MED = (18, (2.0, 10.0, 100.0))
# thin AND tall: young scarps (2 c <= 10.4 taps across) of scale 50 / 100 close to angle 0 - rows of a dozen taps, 100 / 200 of
# them: the kernels without the shared form, staged in several slabs
THIN_MID, THIN_TALL = (50, (1.0, 2.0, 5.0)), (100, (1.0, 2.0, 5.0))
NEAR0 = (-0.2, 0.0, 0.15)
RICK = (9, (1.0, 2.0, 4.0))          # (d = 9: rows of 2 d = 18 taps at +-pi/2 - long runs at every angle)
RICK_L = (30, (0.25, 0.5, 1.0))


def case(name, dem, family, sp, angles, classes, batched, slabs, variant=0, batch_off=False, narrow=False):
    return dict(name=name, dem=dem, family=family, scale=sp[0], params=tuple(sp[1]), angles=tuple(angles), variant=variant,
                batch_off=batch_off, classes=set(classes), batched=batched, slabs=slabs, narrow=narrow)


# classes: every class some launch of the case takes, and no other; batched: some launch carries several orientations;
# slabs: "one" (every template staged whole) or "multi" (some template in several slabs)
CASES = [
    # ---- <1,1>: 256 x 8, always batched
    case("A scarp small <1,1,S> narrow", "A", "scarp", SMALL, ANG, [C11S], True, "one", narrow=True),
    case("B scarp small <1,1,S> narrow", "B", "scarp", SMALL, ANG, [C11S], True, "one", narrow=True),
    case("A upper small <1,1,S> narrow", "A", "upper", SMALL, ANG, [C11S], True, "one", narrow=True),
    case("B ricker <1,1,S> narrow", "B", "ricker", RICK, ANG, [C11S], True, "one", narrow=True),
    case("A ricker <1,1,S> narrow", "A", "ricker", RICK, ANG, [C11S], True, "one", narrow=True),
    case("A scarp thin <1,1> narrow", "A", "scarp", THIN, ANG, [C11], True, "one", narrow=True),
    case("B scarp small v11 <1,1> narrow", "B", "scarp", SMALL, ANG, [C11], True, "one", variant=11, narrow=True),
    # ---- 1030 x 1031: W4 and <1,2>, batched
    case("M scarp small W4,S", "M", "scarp", SMALL, ANG, [W4S], True, "one"),
    case("M upper small W4,S", "M", "upper", SMALL, ANG, [W4S], True, "one"),
    case("M ricker W4,S", "M", "ricker", RICK, ANG, [W4S], True, "one"),
    case("M scarp thin W4", "M", "scarp", THIN, ANG, [W4], True, "one"),
    case("M scarp small v11 W4", "M", "scarp", SMALL, ANG, [W4], True, "one", variant=11),
    case("M scarp small v19 <1,2,S>", "M", "scarp", SMALL, ANG, [C12S], True, "one", variant=19),
    case("M scarp thin v19 <1,2>", "M", "scarp", THIN, ANG, [C12], True, "one", variant=19),
    case("M scarp large <1,2,S> multi-slab", "M", "scarp", LARGE, ANG, [C12S], True, "multi"),
    case("M scarp medium <1,2,S>", "M", "scarp", MED, ANG, [C12S], True, "one"),
    case("M upper large <1,2,S>", "M", "upper", LARGE, OBL, [C12S], True, "one"),
    case("M ricker large <1,2,S>", "M", "ricker", RICK_L, ANG, [C12S], True, "one"),
    case("M scarp large v11 <1,2> multi-slab", "M", "scarp", LARGE, ANG, [C12], True, "multi", variant=11),
    case("M scarp tall <1,2,S> multi-slab", "M", "scarp", TALL, OBL, [C12S], True, "multi"),
    case("M scarp small W4,S batch off", "M", "scarp", SMALL, ANG, [W4S], False, "one", batch_off=True),
    case("M scarp thin W4 batch off", "M", "scarp", THIN, ANG, [W4], False, "one", batch_off=True),
    case("M scarp medium oblique <1,2,S>", "M", "scarp", MED, OBL, [C12S], True, "one"),
    case("M scarp medium oblique <1,2,S> batch off", "M", "scarp", MED, OBL, [C12S], False, "one", batch_off=True),
    case("M scarp thin-tall <1,2> multi-slab", "M", "scarp", THIN_TALL, NEAR0, [C12], True, "multi"),
    case("M scarp thin-tall <1,2> multi-slab batch off", "M", "scarp", THIN_TALL, NEAR0, [C12], False, "multi", batch_off=True),
    # ---- 4091 x 200: one patch column, narrower than the slab
    case("N scarp small W4,S narrow", "N", "scarp", SMALL, ANG, [W4S], True, "one", narrow=True),
    case("N ricker W4,S narrow", "N", "ricker", RICK, ANG, [W4S], True, "one", narrow=True),
    case("N scarp small v19 <1,2,S> narrow", "N", "scarp", SMALL, ANG, [C12S], True, "one", variant=19, narrow=True),
    case("N upper small v11 W4 narrow", "N", "upper", SMALL, ANG, [W4], True, "one", variant=11, narrow=True),
    # ---- 1500 x 1501: W4 and <1,2>, one orientation per launch
    case("U scarp small W4,S", "U", "scarp", SMALL, ANG, [W4S], False, "one"),
    case("U scarp thin W4", "U", "scarp", THIN, ANG, [W4], False, "one"),
    case("U upper small v19 <1,2,S>", "U", "upper", SMALL, ANG, [C12S], False, "one", variant=19),
    case("U scarp large <1,2,S> multi-slab", "U", "scarp", LARGE, ANG, [C12S], False, "multi"),
    case("U scarp medium <1,2,S>", "U", "scarp", MED, OBL, [C12S], False, "one"),
    case("U ricker large v11 <1,2>", "U", "ricker", RICK_L, ANG, [C12], False, "one", variant=11),
    # ---- 2050 x 2061: <2,2>; W4 by default for small boxes; <1,2> by variant 16
    case("L scarp large <2,2,S> multi-slab", "L", "scarp", LARGE, ANG, [C22S], False, "multi"),
    case("L upper large <2,2,S> multi-slab", "L", "upper", LARGE, OBL, [C22S], False, "multi"),
    case("L ricker large <2,2,S> multi-slab", "L", "ricker", RICK_L, ANG, [C22S], False, "multi"),
    case("L scarp large v11 <2,2> multi-slab", "L", "scarp", LARGE, ANG, [C22], False, "multi", variant=11),
    case("L scarp tall <2,2,S> multi-slab", "L", "scarp", TALL, OBL, [C22S], False, "multi"),
    case("L scarp small v19 <2,2,S>", "L", "scarp", SMALL, ANG, [C22S], False, "one", variant=19),
    case("L scarp thin v19 <2,2>", "L", "scarp", THIN, ANG, [C22], False, "one", variant=19),
    case("L scarp small W4,S", "L", "scarp", SMALL, ANG, [W4S], False, "one"),
    case("L scarp large v16 <1,2,S> multi-slab", "L", "scarp", LARGE, ANG, [C12S], False, "multi", variant=16),
    case("L scarp thin W4", "L", "scarp", THIN, ANG, [W4], False, "one"),
    case("L scarp thin-tall <2,2> multi-slab", "L", "scarp", THIN_TALL, NEAR0, [C22], False, "multi"),
    case("L scarp thin-tall v16 <1,2> multi-slab", "L", "scarp", THIN_TALL, NEAR0, [C12], False, "multi", variant=16),
    case("L scarp thin-mid <2,2> multi-slab", "L", "scarp", THIN_MID, NEAR0, [C22], False, "multi"),
    case("L scarp thin-mid v16 <1,2>", "L", "scarp", THIN_MID, NEAR0, [C12], False, "one", variant=16),
    # ---- 8201 x 500: <2,2> on one partial patch column, narrower than the slab
    case("V scarp large <2,2,S> multi-slab narrow", "V", "scarp", LARGE, ANG, [C22S], False, "multi", narrow=True),
    case("V ricker v19 <2,2,S> narrow", "V", "ricker", RICK, ANG, [C22S], False, "one", variant=19, narrow=True),
    case("V upper small v19 <2,2,S> narrow", "V", "upper", SMALL, ANG, [C22S], False, "one", variant=19, narrow=True),
]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)

# Class independence: the two cases of a pair are ONE search (DEM, family, parameters, angles) that the option "variant"
# or "batch" sends through two classes, two slab counts or two batch regimes - the records must be the same bits
# (tests/test_gpu_direct_classes.py).  The shared form on (",S") and off for every kind of pair.
PAIRS = [
    ("L scarp small W4,S", "L scarp small v19 <2,2,S>"),                              # W4 against <2,2>
    ("L scarp thin W4", "L scarp thin v19 <2,2>"),
    ("L scarp large <2,2,S> multi-slab", "L scarp large v16 <1,2,S> multi-slab"),     # <2,2> against <1,2>, large windows
    ("L scarp thin-tall <2,2> multi-slab", "L scarp thin-tall v16 <1,2> multi-slab"),
    ("L scarp thin-mid <2,2> multi-slab", "L scarp thin-mid v16 <1,2>"),              # several slabs against one
    ("M scarp small W4,S", "M scarp small v19 <1,2,S>"),                              # W4 against <1,2>
    ("M scarp thin W4", "M scarp thin v19 <1,2>"),
    ("M scarp small W4,S", "M scarp small W4,S batch off"),                           # batched against one by one
    ("M scarp thin W4", "M scarp thin W4 batch off"),
    ("M scarp medium oblique <1,2,S>", "M scarp medium oblique <1,2,S> batch off"),
    ("M scarp thin-tall <1,2> multi-slab", "M scarp thin-tall <1,2> multi-slab batch off"),
]
# ... and of the uploaded windows (always the shared form): one slab against several, W4 against the whole LDS
WINDOW_PAIRS = [
    ("L tall 100 <2,2,S> multi-slab", "L tall 100 v16 <1,2,S>"),
    ("M tall 56 W4,S", "M tall 56 v19 <1,2,S>"),
]


def window_case(name, dem, make, classes, slabs, variant=0):
    """A search of ONE host-uploaded window, ``make()`` (taken as long runs: direct_long_runs; one orientation)."""
    return dict(name=name, dem=dem, make=make, variant=variant, classes=set(classes), batched=False, slabs=slabs,
                narrow=False, batch_off=False)


def descriptors(c):
    """grid_descriptors of a case on its DEM: arrays of shape (n_angles, n_params)."""
    ny, nx, _ = DEMS[c["dem"]]
    g = WT.grid_descriptors(FAMILIES[c["family"]][0], c["scale"], list(c["params"]), list(c["angles"]), nx, ny, 1.0)
    assert g is not None
    return g


def boxes(c):
    """(wh, ww) of every template, (n_angles, n_params) each, and the union's (pmin, pmax, qmin, qmax)."""
    g = descriptors(c)
    wh = np.asarray(g["pmax"]) - np.asarray(g["pmin"]) + 1
    ww = np.asarray(g["qmax"]) - np.asarray(g["qmin"]) + 1
    bbox = (min(0, int(np.min(g["pmin"]))), max(0, int(np.max(g["pmax"]))), min(0, int(np.min(g["qmin"]))), max(0, int(np.max(g["qmax"]))))
    return wh, ww, bbox


def max_taps(c):
    """The largest support of a case, in taps: the lattice points of a built-in window's c x d rectangle, at most its
    box (Matcher.describe's estimate)."""
    g = descriptors(c)
    wh, ww, _ = boxes(c)
    if c["family"] == "ricker":
        return int((wh * ww).max())
    return int(np.minimum(wh * ww, (2 * np.asarray(g["c"]) + 1) * (2 * np.asarray(g["d"]) + 1)).max())


def reach(c):
    """Cells the case's widest template reaches from its centre, on either axis."""
    return max(abs(v) for v in boxes(c)[2])


def long_run_queries(c):
    """One line per template for the host program: `L <angle index> <param index> <uploaded> <c> <d> <cos> <sin> <dx>`."""
    g = descriptors(c)
    out = []
    for ib in range(len(c["angles"])):
        for ia in range(len(c["params"])):
            out.append("L %d %d 0 %.17g %.17g %.17g %.17g 1.0" % (ib, ia, g["c"][ib, ia], g["d"][ib, ia], g["cos_a"][ib, ia], g["sin_a"][ib, ia]))
    return out


def chunks(c, long_of_run, want):
    """The launches of a case as match_impl lays them out: [(first angle, nb, long_runs)].  ``long_of_run[ib]``: some
    template of orientation ib has long runs; ``want``: direct_batch_want of the DEM.  (At most 32 orientations, one
    family: equal run lengths, parities and mask kinds - consecutive runs of equal `long_runs` ride together.)"""
    n = len(c["angles"])
    assert n <= 32
    out, r = [], 0
    while r < n:
        nb = 1
        if want > 1 and not c["batch_off"]:
            while r + nb < n and long_of_run[r + nb] == long_of_run[r]:
                nb += 1
        out.append((r, nb, bool(long_of_run[r])))
        r += nb
    return out


def route_queries(c, long_of_run, want):
    """One line per (launch, template) for the host program:
    `R <launch> <ch> <cw> <wh_max> <ww_max> <long_runs> <variant> <wh> <ww>`, and the launches."""
    ny, nx, _ = DEMS[c["dem"]]
    if "make" in c:
        wh, ww = cropped_shape(c["make"]())
        return ["R 0 %d %d %d %d 1 %d %d %d" % (ny, nx, wh, ww, c["variant"], wh, ww)], [(0, 1, True)]
    wh, ww, _ = boxes(c)
    ch = chunks(c, long_of_run, want)
    out = []
    for k, (r, nb, lr) in enumerate(ch):
        whm, wwm = int(wh[r:r + nb].max()), int(ww[r:r + nb].max())
        for ib in range(r, r + nb):
            for ia in range(len(c["params"])):
                out.append("R %d %d %d %d %d %d %d %d %d" % (k, ny, nx, whm, wwm, int(lr), c["variant"], wh[ib, ia], ww[ib, ia]))
    return out, ch


# ---- probe windows ---------------------------------------------------------------------------------------------------
def probe_windows(c):
    """[(label, (i0, i1, j0, j1), live)] on the case's DEM: where a class's indexing can break.  Heights and widths keep
    the DEM's parity (the oracle's crop must).  ``live``: the window lies inside every template's window limits - the
    corner, last-patch and border windows do not for the Scarp family, whose cells there are masked for some or all
    templates (the zero record is what is checked); the Ricker family has no window limits, every window is live."""
    ny, nx, _ = DEMS[c["dem"]]
    g = descriptors(c)
    ilo, ihi, jlo, jhi = (np.asarray(g[k]) for k in ("ilo", "ihi", "jlo", "jhi"))
    h, w = 4 + ny % 2, 4 + nx % 2
    hs = 16 + ny % 2
    out = []

    def add(label, i0, j0, hh=h, ww_=w):
        i0, j0 = int(min(max(i0, 0), ny - hh)), int(min(max(j0, 0), nx - ww_))
        win = (i0, i0 + hh, j0, j0 + ww_)
        live = bool(i0 >= ilo.max() and i0 + hh - 1 <= ihi.min() and j0 >= jlo.max() and j0 + ww_ - 1 <= jhi.min())
        out.append((label, win, live))

    # the four corners: the slab wraps on both axes
    add("corner 00", 0, 0)
    add("corner 0x", 0, nx - w)
    add("corner y0", ny - h, 0)
    add("corner yx", ny - h, nx - w)
    # patch seams in y: rows 16 k - 4 .. 16 k + 12 around the middle - the 16-row seam at 16 k, the 8-row seam (the
    # next wave of a two-row class) at 16 k + 8; in x: the column seams nearest the middle
    iy = 16 * (ny // 32)
    xs = sorted({256 * k for k in range(1, (nx - 1) // 256 + 1)}, key=lambda s: (abs(s - nx // 2), s))[:2]
    jmid = nx // 2 - 20
    add("seam y %d|%d, %d|%d" % (iy - 1, iy, iy + 7, iy + 8), iy - 4, jmid, hs)
    for s in xs:
        kind = "512-patch seam" if s % 512 == 0 else "256 seam (the +256 block of a 512 patch)"
        add("seam x %d|%d: %s" % (s - 1, s, kind), iy - 4, s - w // 2, hs)
    # the partial last patch in x (its last columns) and in y (its last rows), away from the corners
    add("last patch x", ny // 3, nx - w)
    add("last patch y", ny - h, nx // 3)
    # astride the window-limit border of the least-limited template, top and left
    add("limit border top", int(ilo.min()) - 2, jmid + 40 if nx > 400 else nx // 2)
    add("limit border left", ny // 2 + 30, int(jlo.min()) - 2)
    add("interior", ny // 2 + 7, nx // 2 + 13)
    return out


# ---- the uploaded windows --------------------------------------------------------------------------------------------
SHARE_MIN = 16                  # SC_DR_SHARE_MIN (sc_direct_route.h); the host program prints it, the host test compares
RUNS_WIDTH = 40


def cropped_shape(W):
    """The box Matcher._describe_generic uploads: the rows and columns between the first and last non-zero weights."""
    nz = np.nonzero(W)
    return int(nz[0].max() - nz[0].min() + 1), int(nz[1].max() - nz[1].min() + 1)


def run_length_rows():
    """[(start, length)] - the rows of the run-length window, top to bottom; (0, 0) is an empty row.  Every length from
    SHARE_MIN - 4 to SHARE_MIN + 8 at every start offset 0 .. 3 within a group of four (lengths below SHARE_MIN: tap by
    tap; from SHARE_MIN: the shared form, whose end-cell pieces depend on start and end modulo 4).  The rows are dealt
    so that the kernel's look-ahead to the next row's first chunk (`pre`) meets every transition: shared after shared,
    tap-by-tap after shared, shared after tap-by-tap, and an empty row in between."""
    lens = list(range(SHARE_MIN - 4, SHARE_MIN + 9))
    shared = [(s, n) for n in lens if n >= SHARE_MIN for s in range(4)]
    plain = [(s, n) for n in lens if n < SHARE_MIN for s in range(4)]
    rows, k = [], 0
    pat = "SSPSESPPS"                               # 5 shared to 3 tap-by-tap (36 to 16 rows), an empty row in nine
    while shared or plain:
        p = pat[k % len(pat)]
        k += 1
        if p == "E":
            rows.append((0, 0))
        elif (p == "S" and shared) or not plain:
            rows.append(shared.pop(0))
        else:
            rows.append(plain.pop(0))
    return rows


def run_length_window(part=None, n_parts=1, holes=(False, True)):
    """The window, (rows, RUNS_WIDTH) float64: the rows of run_length_rows as single hole-free runs; an empty row; then the
    same rows with one hole punched in each (none of those takes the shared form).  Weights vary along and across the
    rows.  ``part`` of ``n_parts``: only that share of the rows (windows short enough for the W4 class), cut so that no
    part begins or ends with an empty row."""
    rows = run_length_rows()
    if part is not None:
        per = -(-len(rows) // n_parts)
        rows = rows[part * per:(part + 1) * per]
        while rows and rows[0] == (0, 0):
            rows = rows[1:]
        while rows and rows[-1] == (0, 0):
            rows = rows[:-1]
    both = []
    for hole in holes:
        if both:
            both.append(np.zeros(RUNS_WIDTH))
        for r, (s, n) in enumerate(rows):
            row = np.zeros(RUNS_WIDTH)
            if n:
                j0 = 8 + s
                row[j0:j0 + n] = np.cos(0.37 * np.arange(n) + 0.9 * r) + 1.3
                if hole:
                    row[j0 + 1 + (r % (n - 2))] = 0.0
            both.append(row)
    return np.array(both)


def tall_window(rows):
    """A window of ``rows`` rows x 21 columns for the slab staging: every fourth row is a hole-free run of 21 taps (the
    shared form; every seventh of those has a hole: tap by tap), the rows between hold four taps, every eleventh row is
    empty.  Weights that change sign along and across the rows.

    (Few taps on purpose.  The kernel's xcorr and T3 are float32 sums over the window's taps in a fixed order; the error
    of such a chain grows with the tap count and with the cancellation in the sum - curvature is a second difference,
    its sum over a box telescopes, so a window with a constant component adds pure cancellation.  A first form of this
    window - 21 taps in every row, weights around 2.0, 3045 taps - measured snr_err 9.1e-05 at 256 x 8, and a plain
    float32 chain over the same taps in numpy gives 8.6e-05: the number format's error, in every class alike, not a slab's.
    This test is about which rows a slab holds; tests/test_direct_classes_host.py holds the windows used here to what a
    float32 chain can deliver, profiles/direct_classes.txt has the figures.)"""
    a, b = np.arange(rows)[:, None], np.arange(21)[None, :]
    W = np.sin(0.9 * a + 0.7 * b) + 0.4 * np.cos(0.23 * a * b) + 0.2
    keep = np.zeros(W.shape, dtype=bool)
    keep[0::4, :] = True
    keep[-1, :] = True
    first = (np.arange(rows) % 5) * 3 + 1
    for r in range(rows):
        keep[r, first[r]:first[r] + 4] = True
    W[~keep] = 0.0
    W[4::28, 9] = 0.0
    W[6::11, :] = 0.0
    assert W[0].all() and W[-1].all()
    return W


def _runs(part=None, n_parts=1, holes=(False, True)):
    return lambda: run_length_window(part, n_parts, holes)


def _tall(rows):
    return lambda: tall_window(rows)


# (On the 1030 x 1031 DEM the run-length window goes in two halves, the single runs and the holed ones, and in three parts
# for the W4 class: a float32 chain's error grows with the tap count, and the largest error of a million cells lies
# further out in the tail than that of the 90 000 of the small DEM - the whole window there measured 6.5e-05.)
# Slabs of a window of 21 columns (pitch 24): 256 x 8 holds 137 of its rows, 256 x 16 whole LDS 129, 512 x 16 60; the W4
# class takes windows of up to 56 rows.  (A window the W4 class takes fits the whole LDS of every class in ONE slab - its
# slab is at most half the LDS, a 512 patch's less than twice a 256 patch's: "one slab against several" is <1,2> against
# <2,2> at 100 rows.)
WINDOW_CASES = [
    window_case("S runs <1,1,S>", "S", _runs(), [C11S], "one"),
    window_case("S runs v11 <1,1>", "S", _runs(), [C11], "one", variant=11),
    window_case("S tall 142 <1,1,S> multi-slab", "S", _tall(142), [C11S], "multi"),
    window_case("S tall 142 v11 <1,1> multi-slab", "S", _tall(142), [C11], "multi", variant=11),
    window_case("M runs single <1,2,S>", "M", _runs(holes=(False,)), [C12S], "one"),
    window_case("M runs holed <1,2,S>", "M", _runs(holes=(True,)), [C12S], "one"),
    window_case("M runs part 0 W4,S", "M", _runs(0, 3), [W4S], "one"),
    window_case("M runs part 1 W4,S", "M", _runs(1, 3), [W4S], "one"),
    window_case("M runs part 2 W4,S", "M", _runs(2, 3), [W4S], "one"),
    window_case("M tall 142 <1,2,S> multi-slab", "M", _tall(142), [C12S], "multi"),
    window_case("M tall 56 W4,S", "M", _tall(56), [W4S], "one"),
    window_case("M tall 56 v19 <1,2,S>", "M", _tall(56), [C12S], "one", variant=19),
    window_case("M tall 56 v11 W4", "M", _tall(56), [W4], "one", variant=11),
    window_case("L tall 100 <2,2,S> multi-slab", "L", _tall(100), [C22S], "multi"),
    window_case("L tall 100 v16 <1,2,S>", "L", _tall(100), [C12S], "one", variant=16),
    window_case("L tall 100 v11 <2,2> multi-slab", "L", _tall(100), [C22], "multi", variant=11),
]
WINDOW_CASE = {c["name"]: c for c in WINDOW_CASES}
assert len(WINDOW_CASE) == len(WINDOW_CASES)


# ---- DEMs and oracle stacks (numpy only) -------------------------------------------------------------------------------
_DEMS, _STACKS = {}, {}
WHOLE = ("A", "B")                    # DEMs small enough for the oracle on every cell (orc.snr_stack)


def dem(name):
    """The DEM of that name, built once (synthetic_scarp with its default noise: a noise floor, report()'s integer policy)."""
    if name not in _DEMS:
        from scarplet_amd import synthetic
        ny, nx, seed = DEMS[name]
        _DEMS[name] = synthetic.synthetic_scarp(nx, seed=seed, ny=ny)
    return _DEMS[name]


def ids(c):
    """(parameter, angle) of every template id: ids are parameter-major (Matcher.describe)."""
    return np.repeat(np.asarray(c["params"], float), len(c["angles"])), np.tile(np.asarray(c["angles"], float), len(c["params"]))


def oracle_windows(c, pool=None):
    """[(label, window, live, amp stack, snr stack)] of a case: the float64 oracle's (T, h, w) stacks, in id order, over
    each probe window - on the small DEMs over the whole grid (orc.snr_stack), on the large ones over crops of the periodic
    DEM with a margin of the templates' reach plus the stencil, which keep the DEM's parity (orc.snr_stack_window).
    Computed once per (DEM, family, scale, parameters, angles) - the variants of a search share it - and read only."""
    import scarplet_oracle as orc
    key = (c["dem"], c["family"], c["scale"], c["params"], c["angles"])
    if key in _STACKS:
        return _STACKS[key]
    g = dem(c["dem"])
    z = np.asarray(g._griddata, dtype=float)
    ny, nx = z.shape
    kind = FAMILIES[c["family"]][1]
    T = len(c["params"]) * len(c["angles"])
    out = []
    if c["dem"] in WHOLE:
        a_st, s_st = orc.snr_stack(z, 1.0, 1.0, kind, c["scale"], list(c["params"]), np.asarray(c["angles"], float))
        out.append(("whole DEM", (0, ny, 0, nx), True, a_st.reshape(T, ny, nx), s_st.reshape(T, ny, nx)))
    else:
        probes = probe_windows(c)
        wins = [w for (_, w, _) in probes]
        margin = reach(c) + 2
        if pool is not None:
            stacks = orc.snr_stack_windows(z, 1.0, 1.0, kind, c["scale"], list(c["params"]), list(c["angles"]), wins, margin, pool)
        else:
            stacks = [orc.snr_stack_window(z, 1.0, 1.0, kind, c["scale"], list(c["params"]), list(c["angles"]), w, margin) for w in wins]
        for (label, w, live), (a_st, s_st) in zip(probes, stacks):
            shape = (T, w[1] - w[0], w[3] - w[2])
            out.append((label, w, live, a_st.reshape(shape), s_st.reshape(shape)))
    for o in out:
        o[3].setflags(write=False)
        o[4].setflags(write=False)
    _STACKS[key] = out
    return out


def check_window(res, c, a_st, s_st):
    """orc.check_fold of a result over one window against its stacks, the project's tolerances (orc.PARITY,
    snr_tolerance of the family, tie_window of the real-space path)."""
    import scarplet_oracle as orc
    kind = FAMILIES[c["family"]][1]
    p_of, a_of = ids(c)
    rtol, afac = orc.snr_tolerance(kind)
    p_amp = orc.PARITY["amp"]
    taps = max_taps(c) if "make" not in c and "scale" in c and len(p_of) > 1 else None
    return orc.check_fold(res, a_st, s_st, p_of, a_of, tie_rtol=orc.tie_window("direct", kind, taps=taps),
                          amp_tol=(p_amp[0], p_amp[1] * np.max(np.abs(a_st))), snr_tol=(rtol, afac * np.max(s_st)))


def merge_checks(chks):
    """One check_fold record for several windows: counts added up, the errors' maxima (what report() prints and judges)."""
    out = dict(chks[0])
    out.pop("ok", None)
    for k in ("n_bad", "n_strict", "n_tie", "n", "n_exact", "n_inexact", "n_below_only", "n_slack", "n_below"):
        out[k] = sum(ch[k] for ch in chks)
    for k in ("inexact_gap", "snr_err", "amp_err"):
        out[k] = max(ch[k] for ch in chks)
    out["exact_frac"] = float(out["n_exact"]) / max(out["n"] - out["n_below_only"], 1)
    return out


def oracle_fold(a_st, s_st, c):
    """The oracle's own fold of a stack: (amp, age, angle, snr) of the argmax template, the zero record where every
    template is masked - the result a perfect device returns."""
    p_of, a_of = ids(c)
    t = np.argmax(s_st, axis=0)
    snr = np.take_along_axis(s_st, t[None], axis=0)[0]
    amp = np.take_along_axis(a_st, t[None], axis=0)[0]
    live = snr > 0
    return np.where(live, amp, 0.0), np.where(live, p_of[t], 0.0), np.where(live, a_of[t], 0.0), snr
