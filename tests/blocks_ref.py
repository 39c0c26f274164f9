"""numpy restatement of seq.kmer.blocks (include/kmhgpu.h), the checker of every blocks test.

The kept segments -- segs_ref.segments(rows, min_len) -- are ordered by (j - i, i); a segment is a
block's head when it is the first of its diagonal or its gap to the segment before it,
i - (previous i + previous len), exceeds max_gap; np.add.reduceat over the heads gives the hits,
the last segment before the next head the span.  Blocks with hits >= min_hits are returned as
(B, 4) int32 {i, j, span, hits}, ordered by (i, j).  The function asserts its own result: every
gap is >= 1, hits <= span, and the hits of all blocks sum to the len of all kept segments."""
import numpy as np

import segs_ref


def merge(segs, max_gap, min_hits=1):
    """The blocks of (S, 3) kept segments {i, j, len} (any order)."""
    g = np.asarray(segs, np.int64).reshape(-1, 3)
    if len(g) == 0:
        return np.zeros((0, 4), np.int32)
    d = g[:, 1] - g[:, 0]
    o = np.lexsort((g[:, 0], d))                      # by diagonal, then i
    g, d = g[o], d[o]
    end = g[:, 0] + g[:, 2]                           # one past the segment's last i
    same = d[1:] == d[:-1]
    gap = g[1:, 0] - end[:-1]
    assert (gap[same] >= 1).all(), "segments of one diagonal touch or overlap"
    head = np.ones(len(g), bool)
    head[1:] = ~same | (gap > max_gap)
    h = np.flatnonzero(head)
    tail = np.r_[h[1:] - 1, len(g) - 1]
    hits = np.add.reduceat(g[:, 2], h)
    span = end[tail] - g[h, 0]
    assert (hits <= span).all() and (span <= 2**31 - 1).all()
    assert hits.sum() == g[:, 2].sum()
    out = np.stack([g[h, 0], g[h, 1], span, hits], axis=1)
    out = out[hits >= min_hits]
    out = out[np.lexsort((out[:, 1], out[:, 0]))]     # by (i, j) of the first row
    return out.astype(np.int32)


def blocks(rows, max_gap, min_len=1, min_hits=1):
    """(B, 4) int32 {i, j, span, hits} of (H, 2) rows, ordered by (i, j)."""
    return merge(segs_ref.segments(rows, min_len), max_gap, min_hits)
