"""reads.kmer.pos and reads.kmer.vote restated from their definitions (include/kmhgpu.h) in plain
Python and numpy, without the library.

reads.kmer.pos is a loop over the reads: the oracle's single query (oracle.OracleIndex, the
compiled reference core) on read_r gives the rows of strand +1, the same query on
revcomp_ref.rc_host(read_r) those of strand -1; reads no longer than k are skipped; `read, strand`
is prepended.  The occurrence cap is maxocc_ref's, applied to each read's rows.

reads.kmer.vote is a dictionary count: a row votes for pos = j - i + k in the cell
(strand, floor(pos / band)); the winner has the most votes, ties go to the forward strand, then to
the smaller bin.  The row definition needs k, so votes_ref takes it."""
import numpy as np

from maxocc_ref import mask_rows
from oracle import oracle as O
from revcomp_ref import rc_host


def _text(r):
    return r if isinstance(r, str) else bytes(r).decode("latin-1")


def rows_ref(index_seq, index_k, reads, k, strands=3, max_occ=0, ox=None) -> np.ndarray:
    """(H, 4) int32 rows (read, strand, i, j).  strands: 1 forward, 2 reverse, 3 both."""
    ox = O.OracleIndex(index_seq, index_k) if ox is None else ox
    out = [np.empty((0, 4), np.int32)]
    for r, read in enumerate(reads, 1):
        read = _text(read)
        if len(read) <= k:
            continue
        for strand, s in ((1, read), (-1, rc_host(read))):
            if not strands & (1 if strand == 1 else 2):
                continue
            ij = mask_rows(index_seq, index_k, ox.query(s, k), max_occ, ox)
            m = np.empty((ij.shape[0], 4), np.int32)
            m[:, 0] = r
            m[:, 1] = strand
            m[:, 2:] = ij
            out.append(m)
    return np.concatenate(out)


def votes_ref(rows, n, k, band) -> np.ndarray:
    """(n, 6) int32 (read, strand, pos, hits, second, total) of any (H, 4) rows."""
    cells = [dict() for _ in range(n)]
    for read, strand, i, j in np.asarray(rows, np.int64).reshape(-1, 4).tolist():
        pos = j - i + k
        key = (strand, pos // band)                  # Python's // floors toward minus infinity
        cells[read - 1][key] = cells[read - 1].get(key, 0) + 1
    out = np.zeros((n, 6), np.int64)
    out[:, 0] = np.arange(1, n + 1)
    for r, c in enumerate(cells):
        if not c:
            continue
        # most votes, then forward (+1 before -1), then the smaller bin
        order = sorted(c.items(), key=lambda kv: (-kv[1], -kv[0][0], kv[0][1]))
        (strand, b), hits = order[0]
        out[r, 1:] = (strand, b * band, hits, order[1][1] if len(order) > 1 else 0,
                      sum(c.values()))
    return out.astype(np.int32)


def pack(reads):
    """(seq uint8, off int64[n + 1]) as DeviceReads packs them."""
    bs = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    off = np.zeros(len(bs) + 1, np.int64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    return np.frombuffer(b"".join(bs), np.uint8).copy(), off
