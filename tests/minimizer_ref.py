"""(w,k)-minimizer sampling restated from its definition (include/kmhgpu.h, kmhg_minimizer_mask),
in plain numpy and not from the library.

Nw = L - k + 1 window starts, 1-based.  valid(s): the oracle's unsampled index holds position s
(OracleIndex.positions), so the window rules (N, the sequence's end) are the oracle's and are not
derived again here.  h(s) = mix64(key(s)) with the key coded from the string (2 bits per char,
(c >> 1) & 3, first char highest) and mix64 written out below.  A span is w consecutive window
starts inside [1, Nw], all valid; window s is selected iff it is the leftmost minimum of h in some
span that contains it.  O(L w): every span is looked at, and np.argmin returns the first minimum.

The reverse strand is the forward rule on rc_host(seq) (tests/revcomp_ref.py)."""
import numpy as np

from oracle import oracle as O
from revcomp_ref import rc_host

_M1 = np.uint64(0xff51afd7ed558ccd)
_M2 = np.uint64(0xc4ceb9fe1a85ec53)
_S = np.uint64(33)


def mix64(h):
    """murmur3's fmix64 on a uint64 array."""
    h = np.asarray(h, np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> _S
        h *= _M1
        h ^= h >> _S
        h *= _M2
        h ^= h >> _S
    return h


def _bytes(seq):
    if isinstance(seq, str):
        return np.frombuffer(seq.encode("latin-1"), np.uint8)
    if isinstance(seq, np.ndarray):
        return seq.astype(np.uint8, copy=False)
    return np.frombuffer(bytes(seq), np.uint8)


def hashes(seq, k):
    """h of every window start (valid or not), uint64[Nw]."""
    b = _bytes(seq)
    nw = len(b) - k + 1
    code = ((b >> 1) & 3).astype(np.uint64)
    key = np.zeros(nw, np.uint64)
    for i in range(k):
        key = (key << np.uint64(2)) | code[i:i + nw]
    return mix64(key)


def valid(seq, k):
    """valid[s - 1] for s in 1 .. Nw: the oracle indexes window s."""
    b = _bytes(seq)
    v = np.zeros(len(b) - k + 1, bool)
    v[O.OracleIndex(b, k).positions.astype(np.int64) - 1] = True
    return v


def mask(seq, k, w, rc=False):
    """uint8[Nw]: entry s - 1 is 1 iff window start s of the strand is selected."""
    b = _bytes(seq)
    if rc:
        b = rc_host(b)
    nw = len(b) - k + 1
    sel = np.zeros(nw, np.uint8)
    if not 1 <= w <= nw:
        return sel
    h, v = hashes(b, k), valid(b, k)
    hw = np.lib.stride_tricks.sliding_window_view(h, w)
    vw = np.lib.stride_tricks.sliding_window_view(v, w)
    t = np.flatnonzero(vw.all(axis=1))               # the spans, by their first window
    sel[t + hw[t].argmin(axis=1)] = 1                # leftmost minimum of each
    return sel


def filter_rows(rows, k, qmask, imask):
    """The (H, 2) rows (i, j) of the unsampled query whose query window (1-based start i - k + 1:
    i is its end) and index window (start j) are both selected, in the unsampled order."""
    rows = np.asarray(rows).reshape(-1, 2)
    i = rows[:, 0].astype(np.int64) - k
    j = rows[:, 1].astype(np.int64) - 1
    return rows[(qmask[i] != 0) & (imask[j] != 0)]
