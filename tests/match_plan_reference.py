"""The search's launch plan (scarplet_amd/csrc/sc_match_plan.h) restated in Python from its rules: what
tests/test_match_plan_host.py holds the header to, field by field, on the lists tests/match_plan_check.cpp prints, and what
tests/test_gpu_match_plan.py counts a search's launches by (``launches``: with the launch shapes of sc_fft_route.h, for the
default options).  No device access.

The rules.  Templates come orientation-major.  A RUN is a stretch of consecutive templates of one orientation (equal cc,
sc2, ss), cut after every 64.  A CHUNK is one run, or a BATCH of consecutive runs that are alike (length, parity, mask
kind; in real space also the long-run flag).  How many: `want` fills the chip; of the alike runs ahead - counted up to the
most one launch sequence holds or two batches and one, whichever is more - a remainder of up to a quarter of `want` rides
along, one below two batches is halved, anything else takes `want`; never more than a launch sequence holds.  Every
chunk lays its windows out from zero, each rounded up to four cells; the real-space rows are padded to four taps.  Kept
spectra: a slot per distinct consecutive orientation, and none at all if some batch does not sit in consecutive slots."""
import collections
import itertools

MAX_GROUP, MAX_BATCH, MAX_ORIENT = 64, 256, 64
SCARP, RICKER, WINDOW = 0, 1, 2
DIRECT, FFT = 0, 1
ERR_FLAGS = 2 | 4
SHARE_MIN = 16.0

In = collections.namedtuple("In", "method to_maps ch cw oy ox dx Ty Tx ntiles group batch_off variant batch_templ batch_fill spectra")
Templ = collections.namedtuple("Templ", "kind flags pmin pmax qmin qmax masked c d cos_a sin_a cc sc2 ss")
Run = collections.namedtuple("Run", "first n parity full long_runs")
Chunk = collections.namedtuple("Chunk", "first n nb wh ww parity full long_runs cells run0")


def up4(v):
    return -(-v // 4) * 4


def fast_rows(inp):
    return inp.Tx in (512, 1024, 2048) and inp.variant != 9


def parity_of(t, inp):
    """1 (odd) for the scarp family, 2 (even) for Ricker - where the support box maps onto itself under the flip."""
    flips = t.pmin + t.pmax == inp.oy - 1 and t.qmin + t.qmax == inp.ox - 1
    return {SCARP: 1, RICKER: 2}.get(t.kind, 0) if flips else 0


def long_rows(t, inp):
    """Window rows of 16 taps or more along x: about min(2 c / |cos|, 2 d / |sin|) cells; an uploaded window: taken as long."""
    if t.kind == WINDOW:
        return True
    across, along = 2.0 * t.c / (abs(t.cos_a) + 1e-9), 2.0 * t.d / (abs(t.sin_a) + 1e-9)
    return min(across, along) / abs(inp.dx) >= SHARE_MIN


def runs_of(inp, templ):
    out, first = [], 0
    for _, same in itertools.groupby(templ, key=lambda t: (t.cc, t.sc2, t.ss)):
        same = list(same)
        for k in range(0, len(same), MAX_GROUP):
            piece = same[k:k + MAX_GROUP]
            par = {parity_of(t, inp) for t in piece}
            out.append(Run(first, len(piece), par.pop() if len(par) == 1 else 0,
                           any(t.flags & ERR_FLAGS or t.masked for t in piece), any(long_rows(t, inp) for t in piece)))
            first += len(piece)
    return out


def want_fft(inp, n):
    """Orientations that fill the chip: the fast row kernel, an orientation's templates in one inverse launch, about 4096
    column workgroups; where three orientations or more fit the row pass's 64 templates the batch stops there, else it may
    carry 256 (option "batch_templ": another number)."""
    if inp.batch_off or n > inp.group or not fast_rows(inp):
        return 1
    cap = inp.batch_templ or MAX_BATCH
    by_table = min(cap, MAX_GROUP) // n if (MAX_GROUP // n >= 3 or cap <= MAX_GROUP) else cap // n
    column_wgs = (inp.ntiles + 1) // 2 * (inp.Tx // 8)
    by_fill = (inp.batch_fill or 4096) // max(column_wgs, 1)
    return max(1, min(by_table, by_fill, MAX_ORIENT))


def want_direct(inp):
    """Small DEMs - up to 1024 patches of 256 x 8 cells - fold 32 orientations per launch."""
    return 32 if -(-inp.cw // 256) * -(-inp.ch // 8) <= 1024 else 1


def batch_of(want, hard, alike_ahead):
    """``alike_ahead(limit)``: this run and the alike ones after it, counted up to ``limit``."""
    if want <= 1:
        return 1
    avail = alike_ahead(max(hard, 2 * want + 1))
    if avail <= want + want // 4:
        nb = avail
    elif avail < 2 * want:
        nb = -(-avail // 2)
    else:
        nb = want
    return min(nb, hard)


def plan(inp, templ):
    """The plan as a dict of the fields match_plan_check prints."""
    runs = runs_of(inp, templ)
    fft = inp.method == FFT
    batching = not inp.to_maps and (fft or (not inp.batch_off and inp.variant != 10))
    n = len(templ)
    win_off, dwin_off, dpitch, span_off = [0] * n, [0] * n, [0] * n, [0] * n
    chunks, r = [], 0
    while r < len(runs):
        a = runs[r]

        def alike(b):
            return (b.n, b.parity, b.full) == (a.n, a.parity, a.full) and (fft or b.long_runs == a.long_runs)

        def alike_ahead(limit):
            k = 1
            while k < limit and r + k < len(runs) and alike(runs[r + k]):
                k += 1
            return k
        nb = 1
        if batching:
            want = want_fft(inp, a.n) if fft else want_direct(inp)
            hard = min(MAX_ORIENT, MAX_BATCH // a.n) if fft else 32
            nb = batch_of(want, hard, alike_ahead)
        cells = dcells = spans = 0
        members = range(a.first, a.first + nb * a.n)
        for j in members:
            h, w = templ[j].pmax - templ[j].pmin + 1, templ[j].qmax - templ[j].qmin + 1
            win_off[j], dwin_off[j], dpitch[j], span_off[j] = cells, dcells, up4(w), spans
            cells = up4(cells + h * w)
            dcells += h * up4(w)
            spans += h
        chunks.append((Chunk(a.first, a.n, nb, max(templ[j].pmax - templ[j].pmin + 1 for j in members),
                             max(templ[j].qmax - templ[j].qmin + 1 for j in members), a.parity, a.full, a.long_runs, cells, r),
                       dcells, spans))
        r += nb
    slot_of, n_slots = [0] * len(runs), 0
    if fft and not inp.to_maps and inp.spectra:
        key = [(templ[q.first].cc, templ[q.first].sc2, templ[q.first].ss) for q in runs]
        for k in range(len(runs)):
            if k and key[k] == key[k - 1]:
                slot_of[k] = slot_of[k - 1]
            else:
                slot_of[k], n_slots = n_slots, n_slots + 1
        for c, _, _ in chunks:
            if slot_of[c.run0:c.run0 + c.nb] != list(range(slot_of[c.run0], slot_of[c.run0] + c.nb)):
                n_slots = 0
    return dict(runs=runs, chunks=[c for c, _, _ in chunks], win_off=win_off, dwin_off=dwin_off, dpitch=dpitch, span_off=span_off,
                max=(max(c.cells for c, _, _ in chunks), max(d for _, d, _ in chunks), max(s for _, _, s in chunks),
                     max(c.nb for c, _, _ in chunks), max(c.nb * c.n for c, _, _ in chunks)),
                n_slots=n_slots, slot_of=slot_of)


# ---- what match_plan_check prints ------------------------------------------------------------------------------------
def parse(text):
    """[(In, [Templ], plan dict)] of the output of `match_plan_check print`."""
    lines = iter(text.split("\n"))
    out = []

    def ints(line, name=None):
        f = line.split()
        if name is not None:
            assert f[0] == name, (f[0], name)
            f = f[1:]
        return [int(v) for v in f]

    for line in lines:
        if not line:
            continue
        assert line.startswith("case "), line
        f = next(lines).split()
        assert f[0] == "in"
        inp = In(*[float(v) if k == 6 else int(v) for k, v in enumerate(f[1:17])])
        templ = []
        for _ in range(int(f[17])):
            f = next(lines).split()
            assert f[0] == "t"
            templ.append(Templ(*([int(v) for v in f[1:8]] + [float(v) for v in f[8:]])))
        got = {}
        got["runs"] = [Run(*[bool(v) if k > 2 else v for k, v in enumerate(ints(next(lines)))]) for _ in range(ints(next(lines), "runs")[0])]
        got["chunks"] = [Chunk(*[bool(v) if k in (6, 7) else v for k, v in enumerate(ints(next(lines)))])
                         for _ in range(ints(next(lines), "chunks")[0])]
        for name in ("win_off", "dwin_off", "dpitch", "span_off"):
            got[name] = ints(next(lines), name)
        got["max"] = tuple(ints(next(lines), "max"))
        s = ints(next(lines), "slots")
        got["n_slots"], got["slot_of"] = s[0], s[1:]
        out.append((inp, templ, got))
    return out


# ---- a search of the Python layer, and its launches --------------------------------------------------------------------
def of_search(matcher, arr, sp, batch_off=False, to_maps=False):
    """(In, [Templ]) of the descriptors ``arr`` (Matcher.describe; built-in classes: no per-cell masks) and the plan ``sp``
    (Matcher.plan_for) on the matcher's context with its default options but "batch"."""
    c = matcher.core
    inp = In(int(sp.method), to_maps, c[1] - c[0], c[3] - c[2], matcher.ny % 2, matcher.nx % 2, float(matcher.dx), int(sp.Ty), int(sp.Tx),
             int(sp.nty) * int(sp.ntx), max(1, int(sp.group)), batch_off, 0, 0, 0, matcher.ctx.spectra_mb > 0)
    templ = [Templ(int(s.kind), int(s.flags), int(s.pmin), int(s.pmax), int(s.qmin), int(s.qmax), False, float(s.c), float(s.d),
                   float(s.cos_a), float(s.sin_a), float(s.cc), float(s.sc2), float(s.ss)) for s in arr]
    return inp, templ


def launches(inp, sp, chunks, near=False):
    """The rise of the launch counters over a search of ``chunks`` (plan()["chunks"]) with the default options (variant 0,
    "i1_pairs" 2, "split_fill" 0, no sibling rendezvous), every tile pair in one hand-off (small tiles: the memory holds
    them): dict of k_windows, k_direct, k_inv_cols, k_inv_rows.  Real space: the windows and their reversed rows, then one
    launch.  FFT: the windows; per tile-pair chunk (the whole pairs; the odd tile alone, templates in pairs) and group of
    templates the column launches - the generic and the small symmetric kernels take two each, own columns and mirrors -
    and the row pass in slices of whole orientations."""
    assert inp.variant == 0 and not inp.to_maps
    out = dict(k_windows=0, k_direct=0, k_inv_cols=0, k_inv_rows=0)
    if inp.method == DIRECT:
        out["k_windows"], out["k_direct"] = 2 * len(chunks), len(chunks)
        return out
    Ty, Tx = inp.Ty, inp.Tx
    pairs = (inp.ntiles + 1) // 2
    rows = Ty // 2 if sp.circ_y else min(Ty - 1, sp.Py + sp.Vy - 1) // 2 - sp.Py // 2 + 1           # row pairs with valid outputs
    fast = fast_rows(inp)
    for c in chunks:
        out["k_windows"] += 1
        sym = c.parity != 0 and Ty <= 2048
        symx = sym and Ty >= 512 and Tx % 64 == 0
        w8 = symx and Ty in (1024, 2048) and Tx % 128 == 0
        odd_alone = sym and fast and inp.ntiles % 2 == 1
        for paired, pc in ((False, pairs - 1 if odd_alone else pairs), (True, 1 if odd_alone else 0)):
            if pc == 0:
                continue
            paired_orient = paired and c.n == 1 and c.nb >= 2 and symx and Ty == 512
            half_wave = symx and Ty == 512 and Tx % 256 == 0
            wave_per_column = not paired_orient and not half_wave and w8 and (not paired or Ty == 1024)
            two_launches = not symx                              # generic, or symmetric below 512 / at odd widths
            dealt = fast and not (near and paired_orient) and not c.full and Tx <= 1024
            for g0 in range(0, c.n, inp.group):
                G = min(inp.group, c.n - g0)
                if wave_per_column and c.nb == 1:
                    per = min(pc, 2)
                elif c.nb > 1:
                    per = pc
                else:
                    lds = 4 * (Ty + Ty // 16 + 8) * 8 + (4 * Ty * 8 if Ty <= 2048 else 0)
                    per = max(1, min(pc, -(-256 * max(1, 160 * 1024 // lds) // (Tx // 8))))
                out["k_inv_cols"] += -(-pc // per) * (2 if two_launches else 1)
                shares = 1
                if dealt and G >= (4 if near else 1):
                    shares = max(1, min(4, (4300 // (Tx // 512)) // max(1, rows * 2 * pc)))
                if c.nb > 1 and not paired_orient:
                    templates = min(255, MAX_GROUP * shares * (2 if paired else 1)) if shares > 1 else MAX_GROUP
                    at_most = -(-c.nb // max(1, templates // G))          # slices; of equal size: so many orientations each
                    slices = -(-c.nb // -(-c.nb // at_most))
                else:
                    slices = 1
                out["k_inv_rows"] += slices
    return out
