"""kmer.pairs restated in plain Python straight from its definition (include/kmhgpu.h), the second
checker of every pairs test beside OracleIndex.pairs_with.

For every k-mer of `a`, in the order `a` first shows them, that `b` also holds: each 1-based start
of it in `a` (outer, ascending) with each start of it in `b` (inner, ascending), as interleaved
int32 (pos_a, pos_b).  The only thing taken from the oracle is its window rule (O.windows: which
windows are valid and their 2-bit keys); the lists, their order and the cross products are dicts
and loops here, nothing else.  A counts index reads the same way with its count vectors in the
place of the start lists (kmer_counts)."""
import numpy as np

from oracle import oracle as O


def kmer_starts(seq, k: int) -> dict:
    """{key: ascending 1-based starts}, the keys in first-occurrence order."""
    keys, starts, _ = O.windows(seq, k)
    d: dict = {}
    for key, s in zip(keys.tolist(), starts.tolist()):
        d.setdefault(key, []).append(s)
    return d


def kmer_counts(calls, k: int, source_n: int) -> dict:
    """{key: [count per source]} after the count.kmers calls [(source, [sequence, ...]), ...], the
    keys in first-insertion order.  Sequences of length <= k are skipped."""
    d: dict = {}
    for source, seqs in calls:
        for seq in seqs:
            if len(seq) <= k:
                continue
            for key in O.windows(seq, k)[0].tolist():
                d.setdefault(key, [0] * source_n)[source] += 1
    return d


def cross(da: dict, db: dict, order=None) -> np.ndarray:
    """The rows of two {key: list} tables; `order`: the ranks of da's keys in visiting order."""
    items = list(da.items())
    if order is not None:
        items = [items[int(r)] for r in order]
    out = []
    for key, la in items:
        lb = db.get(key)
        if lb is None:
            continue
        for x in la:
            for y in lb:
                out.append(x)
                out.append(y)
    return np.array(out, np.int32)


def pairs_ref(a, b, k: int, order=None) -> np.ndarray:
    return cross(kmer_starts(a, k), kmer_starts(b, k), order)


def key_counts(a, b, k: int) -> list:
    """(key, count in a, count in b) for every k-mer of `a` in first-occurrence order."""
    da, db = kmer_starts(a, k), kmer_starts(b, k)
    return [(key, len(la), len(db.get(key, ()))) for key, la in da.items()]
