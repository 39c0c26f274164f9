"""numpy restatement of seq.kmer.segs (include/kmhgpu.h), the checker of every segments test.

rows: the (H, 2) int32 (i, j) rows of a seq.kmer.pos result, i, j >= 1, strictly ascending by
(i, j).  A segment (i, j, len) is a maximal diagonal stretch of the rows.  Membership is a
searchsorted on the key i << 32 | j (uint64: i + 1 may be 2^31); starts and ends are paired per
diagonal by a lexsort on (j - i, i).  The function asserts its own result: the lengths sum to the
row count and the segments expand back to exactly the rows."""
import numpy as np


def _key(i, j):
    return (i.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)


def expand(segs):
    """The rows of (S, 3) segments, sorted by (i, j), as an (H, 2) int32 array."""
    segs = np.asarray(segs, np.int64).reshape(-1, 3)
    n = segs[:, 2]
    if n.sum() == 0:
        return np.zeros((0, 2), np.int32)
    first = np.repeat(np.cumsum(n) - n, n)
    t = np.arange(n.sum()) - first
    i = np.repeat(segs[:, 0], n) + t
    j = np.repeat(segs[:, 1], n) + t
    o = np.argsort(_key(i, j), kind="stable")
    return np.stack([i[o], j[o]], axis=1).astype(np.int32)


def segments(rows, min_len=1):
    """(S, 3) int32 {i, j, len}, ordered by (i, j) of the first row, len >= min_len."""
    r = np.asarray(rows, np.int64).reshape(-1, 2)
    if len(r) == 0:
        return np.zeros((0, 3), np.int32)
    assert (r >= 1).all() and (r <= 2**31 - 1).all()
    key = _key(r[:, 0], r[:, 1])
    assert (key[1:] > key[:-1]).all(), "rows not strictly ascending by (i, j)"

    def member(i, j):
        k = _key(i, j)
        p = np.minimum(np.searchsorted(key, k), len(key) - 1)
        return key[p] == k

    start = ~member(r[:, 0] - 1, r[:, 1] - 1)        # (a zero coordinate is never a row)
    end = ~member(r[:, 0] + 1, r[:, 1] + 1)
    s, e = r[start], r[end]
    assert len(s) == len(e)
    os_ = np.lexsort((s[:, 0], s[:, 1] - s[:, 0]))   # by diagonal, then i
    oe = np.lexsort((e[:, 0], e[:, 1] - e[:, 0]))
    assert np.array_equal((s[:, 1] - s[:, 0])[os_], (e[:, 1] - e[:, 0])[oe])
    ln = np.empty(len(s), np.int64)
    ln[os_] = e[oe, 0] - s[os_, 0] + 1
    assert (ln >= 1).all() and ln.sum() == len(r)
    out = np.stack([s[:, 0], s[:, 1], ln], axis=1).astype(np.int32)
    assert np.array_equal(expand(out), r.astype(np.int32))
    return out[ln >= min_len]
