"""count.kmers.fq.sh's k-mer walk as a clean-room automaton, written from the rules of the walk
(include/kmhgpu.h, "single-source read counting") and not from the reference's text: a second
opinion beside tests/ref_fq_sh.py and the source of expected keys for seeded inputs.

Per base of a record, with mq = (char)(min_quality + '!') and signed char comparisons:
    bad   N / n, or qual < mq        weak  not N and qual == mq        good  not N and qual > mq
FASTA records (qual None): only N is bad, nothing is weak.  A NUL ends the record.
"""
from collections import Counter

_CODE = {c: (c >> 1) & 3 for c in range(256)}


def threshold_char(min_quality: int) -> int:
    """(char)(min_quality + '!') as a signed value."""
    v = (min_quality + 33) & 0xFF
    return v - 256 if v >= 128 else v


def _schar(b: int) -> int:
    return b - 256 if b >= 128 else b


def classify(seq: bytes, qual, mq: int) -> str:
    """One letter per base up to the first NUL: 'b'ad, 'w'eak, 'g'ood."""
    end = seq.find(b"\0")
    n = len(seq) if end < 0 else end
    out = []
    for i in range(n):
        if seq[i] | 0x20 == 0x6E:
            out.append("b")
        elif qual is None:
            out.append("g")
        else:
            q = _schar(qual[i])
            out.append("b" if q < mq else ("w" if q == mq else "g"))
    return "".join(out)


def canonical(seq: bytes, p: int, k: int) -> int:
    f = 0
    r = 0
    for j in range(k):
        c = _CODE[seq[p + j]]
        f = (f << 2) | c
        r |= ((c + 2) & 3) << (2 * j)
    return min(f, r)


def window_starts(cls: str, k: int) -> list:
    """Start positions of the windows the walk counts, in walk order."""
    n = len(cls)
    out = []
    s = 0
    while s < n:
        # init from s: k consecutive non-bad bases; a bad base moves the start past its bad run
        j = s
        while j < n and j - s < k and cls[j] != "b":
            j += 1
        if j - s < k:
            if j >= n:
                break                      # the record ends inside the attempt
            while j < n and cls[j] == "b":
                j += 1
            s = j
            continue
        if j == n:
            break                          # the window ends the record: nothing is counted
        out.append(s)
        e = j                              # roll: every following good base
        while e < n and cls[e] == "g":
            out.append(e - k + 1)
            e += 1
        s = e                              # a weak base starts the next init, a bad one is skipped
    return out


def record_keys(seq: bytes, qual, k: int, min_quality: int) -> list:
    cls = classify(seq, qual, threshold_char(min_quality))
    return [canonical(seq, p, k) for p in window_starts(cls, k)]


def count_records(records, k: int, min_quality: int, max_read_n: int = -1) -> Counter:
    """records: iterable of (seq, qual or None).  The first max_read_n are taken (negative: all),
    those no longer than k skipped."""
    limit = max_read_n if max_read_n >= 0 else 1 << 62
    c = Counter()
    for i, (s, q) in enumerate(records):
        if i >= limit:
            break
        if len(s) <= k:
            continue
        c.update(record_keys(s, q, k, min_quality))
    return c


def spectrum(counts: Counter, max_count: int) -> list:
    out = [0.0] * (max_count + 1)
    for v in counts.values():
        out[min(v, max_count)] += 1.0
    return out
