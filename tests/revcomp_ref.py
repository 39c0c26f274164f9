"""rc_host: the reverse complement seq.kmer.pos.rc queries, written from its definition
(include/kmhgpu.h, kmhg_query_run_rc) and not from the library.  For p in [0, L):

    rc(S)[p] = 'N'                                 if S[L-1-p] is 'N' or 'n'
             = "ACTG"[((S[L-1-p] >> 1) & 3) ^ 2]   otherwise

The checker of every rc test is the forward oracle on rc_host(S)."""
import numpy as np

_TABLE = np.array([ord("N") if (c | 0x20) == ord("n") else b"ACTG"[((c >> 1) & 3) ^ 2]
                   for c in range(256)], np.uint8)


def rc_host(seq):
    """bytes / str / uint8 array -> the same type, reverse-complemented."""
    if isinstance(seq, np.ndarray):
        return _TABLE[seq[::-1]]
    if isinstance(seq, str):
        return rc_host(seq.encode("latin-1")).decode("latin-1")
    return _TABLE[np.frombuffer(bytes(seq), np.uint8)[::-1]].tobytes()
