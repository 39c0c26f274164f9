"""kmer.max.occ restated on the oracle's rows (include/kmhgpu.h, kmhg_set_max_occ): the rows of
seq.kmer.pos whose indexed k-mer occurs more than max_occ times in the index are deleted, and
nothing else changes -- not the order, not the other rows.  A row (i, j) names the indexed window
that starts at j (1-based), whose k-mer is a[j - 1 : j - 1 + k]; how often that k-mer occurs is
the oracle's own kmer.pos count of it (OracleIndex.counts), so the window rules (N, the sequence's
end) are the oracle's and are not derived again here."""
import numpy as np

from oracle import oracle as O


COUNTS = [1, 2, 4, 5, 255, 257, 2100]        # around the caps tried, the emit's direct / dealt split
TILE = 2048


def counted_case(k=15):
    """The counted index of tests/test_gpu_segrec.py: each unit (k + 5 chars: 6 windows) repeated c
    times, copies separated by N, so a query window of the unit has exactly c hits.  The query is
    every unit, random filler that hits nothing, and -- in a second 2,048-window tile -- the units
    of 1, 5 and 2,100 hits again: with a cap of 4 that tile's multi-hit windows are all masked and
    its single hits stay.  Returns (k, units, a, query, OracleIndex(a, k))."""
    from kmer_hasher_amd import synth
    rng = np.random.default_rng(123)
    units = ["".join(rng.choice(list("ACGT"), k + 5)) for _ in COUNTS]
    a = "".join((u + "N") * c for u, c in zip(units, COUNTS))
    head = "N".join(units) + "N"
    tail = "N" + units[0] + "N" + units[3] + units[6][:k]      # the last window hits
    nw = TILE + 777
    fill = synth.iid(nw + k - 1 - len(head) - len(tail), 2900).tobytes().decode()
    return k, units, a, head + fill + tail, O.OracleIndex(a, k)


def occurrences(ox) -> np.ndarray:
    """occ[j] = the kmer.pos count of the k-mer indexed at position j (1-based), 0 where the oracle
    indexes no window."""
    occ = np.zeros(int(ox.positions.max(initial=0)) + 2, np.int64)
    occ[ox.positions] = np.repeat(ox.counts.astype(np.int64), ox.counts)
    return occ


def mask_rows(a, k, rows, max_occ, ox=None) -> np.ndarray:
    """The (H, 2) rows (i, j) of a query against the index of `a` at k, without the rows whose
    indexed k-mer occurs more than max_occ times in `a`; max_occ = 0 deletes nothing.  `ox`: the
    OracleIndex of (a, k) where the caller has it already."""
    rows = np.asarray(rows).reshape(-1, 2)
    if max_occ == 0:
        return rows
    occ = occurrences(O.OracleIndex(a, k) if ox is None else ox)
    n = occ[rows[:, 1]]
    assert (n >= 1).all()                            # every row points at an indexed window
    return rows[n <= max_occ]
