"""seq.kmer.chains restated in plain numpy, O(B^2), from the definition in include/kmhgpu.h (not
from the kernels): every block looks at every other block for its predecessor.  Every chains test
checks against `chains`; it asserts its own result (at most one link in and one link out per
block, chain blocks strictly increasing in i and j, the hit and block sums)."""
import numpy as np

M = 2**31 - 1


def check_blocks(blocks):
    """The (B, 4) int64 blocks, asserted to be what seq.kmer.blocks returns."""
    b = np.asarray(blocks, np.int64).reshape(-1, 4)
    i, j, span, hits = b.T
    assert (i >= 1).all() and (j >= 1).all() and (span >= 1).all()
    assert (hits >= 1).all() and (hits <= span).all()
    assert (i + span - 1 <= M).all() and (j + span - 1 <= M).all()
    if len(b) > 1:
        assert ((i[1:] > i[:-1]) | ((i[1:] == i[:-1]) & (j[1:] > j[:-1]))).all(), "not ascending"
    return b


def links(blocks, max_dist, max_drift):
    """(pred, child): pred[b] = the block b chose (-1: none), child[a] = the block that won a."""
    b = check_blocks(blocks)
    B = len(b)
    i, j, span, _ = b.T
    ei, ej = i + span - 1, j + span - 1
    pred = np.full(B, -1, np.int64)
    cost = np.zeros(B, np.int64)
    for t in range(B):
        gi, gj = i[t] - ei - 1, j[t] - ej - 1
        ok = (gi >= 0) & (gj >= 0) & (np.maximum(gi, gj) <= max_dist) & \
            (np.abs(gj - gi) <= max_drift)
        cand = np.flatnonzero(ok)
        if len(cand):
            c = gi[cand] + gj[cand]
            assert c.max() < 2**32
            pred[t] = cand[c == c.min()][0]          # the smallest cost << 32 | a
            cost[t] = c.min()
    child = np.full(B, -1, np.int64)
    for t in range(B):                               # ascending b: a tie goes to the lower b
        a = pred[t]
        if a >= 0 and (child[a] < 0 or cost[t] < cost[child[a]]):
            child[a] = t
    return pred, child


def chains(blocks, max_dist, max_drift, min_hits=1):
    """((C, 6) int32 chains {i, j, i.end, j.end, hits, blocks}, (B,) int32 chain[b])."""
    b = check_blocks(blocks)
    B = len(b)
    pred, child = links(b, max_dist, max_drift)
    idx = np.arange(B)
    link_in = (pred >= 0) & (child[np.maximum(pred, 0)] == idx)      # pred(b) = a, child(a) = b
    nxt = np.where((child >= 0) & (pred[np.maximum(child, 0)] == idx), child, -1)
    assert np.array_equal(np.sort(nxt[nxt >= 0]), np.flatnonzero(link_in))   # one in, one out
    assert len(np.unique(nxt[nxt >= 0])) == (nxt >= 0).sum()
    i, j, span, hits = b.T
    ei, ej = i + span - 1, j + span - 1
    recs, owner, first = [], np.full(B, -1, np.int64), []
    for h in np.flatnonzero(~link_in):               # the (i, j) order of the first blocks
        t, n, total = h, 0, 0
        while True:
            assert owner[t] < 0
            owner[t] = len(recs)
            n += 1
            total += hits[t]
            if nxt[t] < 0:
                break
            assert i[nxt[t]] > ei[t] and j[nxt[t]] > ej[t]           # strictly increasing
            t = nxt[t]
        assert total < 2**31
        recs.append((i[h], j[h], ei[t], ej[t], total, n))
        first.append(h)
    assert (owner >= 0).all()
    r = np.asarray(recs, np.int64).reshape(-1, 6)
    assert r[:, 4].sum() == hits.sum() and r[:, 5].sum() == B
    keep = r[:, 4] >= min_hits
    number = np.where(keep, np.cumsum(keep), 0)      # 1-based among the kept chains
    member = number[owner] if B else np.zeros(0, np.int64)
    return r[keep].astype(np.int32), member.astype(np.int32)
