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


BLOCK = 64            # SG_BLOCK: usable profiles per block of the segmented sum


def chunk_arrays(seg_start, s0, s1):
    """What the host sends up of the chunk of segments s0..s1, its cells counted from its first: (start, blk, cseg, G) - the
    CSR array of the cells over the chunk's segments, that of the blocks of 64 cells, the segment of every cell, and the
    number of blocks."""
    import numpy as np
    start = np.asarray(seg_start[s0:s1 + 1], dtype=np.int64) - seg_start[s0]
    size = np.diff(start)
    blk = np.concatenate([[0], np.cumsum(-(-size // BLOCK))])
    return start, blk, np.repeat(np.arange(s1 - s0), size), int(blk[-1])


def block_totals(seg_start):
    """The CSR array of the block totals of the call with max_width over all segments: a segment's blocks and one more."""
    import numpy as np
    return np.concatenate([[0], np.cumsum(-(-np.diff(np.asarray(seg_start, dtype=np.int64)) // BLOCK) + 1)])


def park_cap(max_park, prof, planes, columns, shift):
    """The cells of one segment that a park of max_park bytes holds: 8 (prof + planes columns) bytes a cell, and one byte a
    column for the shifts."""
    return max_park // (8 * (prof + planes * columns) + (columns if shift else 0))
