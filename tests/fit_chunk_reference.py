"""The chunk rule of the fit drivers (scarplet_amd/csrc/sc_fit_chunk.h, option "fit_chunk") restated in Python: what
tests/test_fit_chunks_host.py holds the header to and what tests/test_gpu_fit_chunks.py counts launches by."""


def bound(cap, n):
    """The cells of a chunk: the built-in bound, lowered - never raised - by the option n > 0."""
    return n if 0 < n < cap else cap


def chunks(seg_start, max_segs, max_cells, aux_start=None, max_aux=0):
    """The boundaries [0, s_1, ..., S] of the chunks of whole segments: a chunk takes its first segment whatever its
    size, then every next one while segments, cells and the items of the second CSR array stay within their bounds."""
    S, cuts = len(seg_start) - 1, [0]
    while cuts[-1] < S:
        s0 = cuts[-1]
        s1 = s0 + 1
        while (s1 < S and s1 + 1 - s0 <= max_segs and seg_start[s1 + 1] - seg_start[s0] <= max_cells
               and (aux_start is None or aux_start[s1 + 1] - aux_start[s0] <= max_aux)):
            s1 += 1
        cuts.append(s1)
    return cuts


def per_cell_chunks(K, chunk, n):
    """Launches of a per-cell call over K cells."""
    c = min(K, bound(chunk, n))
    return 0 if K == 0 else -(-K // c)
