"""Packed read batches for the device entries of read counting (kmhg_sh_count_reads_device,
kmhg_sh1_count_reads_device): ragged lengths, record arrays that do not start at offset 0, FASTA
records laid against k_fa_kmers' tile edges -- and the host-side predicates that say which kernel
branch a batch reaches, computed from the offsets alone as the kernels compute them.
Deterministic; shared by tests/test_packed_inputs.py (CPU) and tests/test_gpu_packed_reads.py.

A batch is (records, seq, qual, off, hasq): records = [(seq bytes, qual bytes or None)], seq / qual
the packed bytes with 16 zero bytes of padding, off int64[n + 1], hasq uint8[n].  Records without
qualities carry zero bytes in qual.
"""
import functools
from collections import Counter

import numpy as np

import fq_walk as W
from fq_sh_inputs import BAD, FA_TILE, GOOD, MQ, WEAK

RK_READS = 64           # k_read_kmers / k_read_kmers_sh1: reads per wave (kmhg_sh.hip)
RK_CAP = 28672          # largest span a wave stages in LDS (read_kmers_cap_span, kmhg_sh.h)
FA_CPT = 16             # k_fa_kmers: window starts per lane (kmhg_sh.h)
MQ_RP = 20              # .rp min_q: windows of 'I' pass, a '#' fails, some '?' are tolerated
SEEDS = {9: 2, 21: 1, 31: 6}    # per k, the seed of every GPU case: chosen so that the reach
                                # conditions of tests/test_packed_inputs.py hold
N_READS = (1, 63, 64, 65, 200)
SHARES = (0.0, 1 / 3, 1.0)
KS = (9, 21, 31)


def lengths(k: int) -> list:
    return [0, 1, k - 1, k, k + 1, k + 2, 2 * k, 150, 151, 700, 5000]


def _bases(rng, n):
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    nn = rng.random(n) < 0.02
    s[nn] = rng.choice(np.frombuffer(b"Nn", np.uint8), int(nn.sum()))
    return s


def _quals(rng, n):
    return rng.choice(np.array([GOOD, WEAK, BAD], np.uint8), n, p=[.9, .06, .04])


def pack(records):
    """(records, seq, qual, off, hasq) of a record list."""
    off = np.zeros(len(records) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s, _ in records])
    seq = np.zeros(int(off[-1]) + 16, np.uint8)
    qual = np.zeros(int(off[-1]) + 16, np.uint8)
    for i, (s, q) in enumerate(records):
        seq[off[i]:off[i + 1]] = np.frombuffer(s, np.uint8)
        if q is not None:
            assert len(q) == len(s)
            qual[off[i]:off[i + 1]] = np.frombuffer(q, np.uint8)
    hasq = np.array([q is not None for _, q in records], np.uint8)
    return records, seq, qual, off, hasq


def ragged_records(seed, k, n_reads, fasta_share, max_len=5000, nuls=True):
    rng = np.random.default_rng([seed, k, n_reads, int(round(fasta_share * 3))])
    lens = [x for x in lengths(k) if x <= max_len]
    w = np.array([8.0 if x == 5000 else 7.0 if x == 700 else 10.0 for x in lens])
    ln = rng.choice(lens, n_reads, p=w / w.sum())
    if fasta_share <= 0:
        fa = np.zeros(n_reads, bool)
    elif fasta_share >= 1:
        fa = np.ones(n_reads, bool)
    else:
        fa = rng.random(n_reads) < fasta_share
    seqs = [_bases(rng, int(x)) for x in ln]
    quals = [None if f else _quals(rng, int(x)) for x, f in zip(ln, fa)]
    # NULs: a record's first byte, its last, the middle, and directly after a full init window
    # (k good bases, then the NUL: the window ends the record).  At least one long record is left
    # whole, so small batches plant none.
    cand = [i for i in range(n_reads) if ln[i] >= 2 * k]
    if nuls and len(cand) >= 5:
        pick = rng.choice(cand, 4, replace=False)
        for i, kind in zip(pick, ("first", "last", "middle", "after_init")):
            s, n = seqs[i], int(ln[i])
            if kind == "after_init":
                s[:k] = rng.choice(np.frombuffer(b"ACGT", np.uint8), k)
                if quals[i] is not None:
                    quals[i][:k] = GOOD
            s[{"first": 0, "last": n - 1, "middle": n // 2, "after_init": k}[kind]] = 0
    return [(s.tobytes(), None if q is None else q.tobytes()) for s, q in zip(seqs, quals)]


def ragged_batch(seed, k, n_reads, fasta_share, max_len=5000, nuls=True):
    """Lengths from lengths(k) (no longer than max_len), ~2 % N/n, qualities GOOD/WEAK/BAD, a few
    NULs; fasta_share of the records without qualities (0 and 1 exactly: none / all)."""
    return pack(ragged_records(seed, k, n_reads, fasta_share, max_len, nuls))


# ---------------------------------------------------------------- sub-ranges of a batch
# name -> (off[i0] % 16, the byte just before off[i0], the record at i0, records before)
SUB_VARIANTS = {
    "rem0_nul": (0, "nul", "fastq_150", 70),
    "rem1_n": (1, "n", "fasta_k1", 70),
    "rem15_plain": (15, "plain", "fasta_k", 70),
    "below16_plain": (5, "plain", "fastq_k", 0),
}


def sub_range_batch(seed, k, variant):
    """(batch, i0, i1): the ragged 200-record batch (a third FASTA) with two records put in after
    `a` records, so that the sub-range [i0, i1) starts at off[i0] = 16 m + rem: a neighbour whose
    last byte is a NUL, an N or a plain good base (its tail would form k-mers with the sub-range's
    first bases if a kernel read across off[i0]), then the sub-range's first record -- with
    qualities (150 or exactly k bases) or FASTA of exactly k / k + 1 N-free bases.  i1 - i0 = 101:
    neither end sits on a wave of 64 reads."""
    rem, before, first, a = SUB_VARIANTS[variant]
    rng = np.random.default_rng([seed, k, 77, rem])
    recs = ragged_records(seed, k, 200, 1 / 3)
    base = sum(len(s) for s, _ in recs[:a])
    n = 2 * k + 16 + (rem - base - 2 * k - 16) % 16 if a else rem
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    s[-1] = {"nul": 0, "n": ord("N"), "plain": s[-1]}[before]
    fasta_first = first.startswith("fasta")
    neighbour = (s.tobytes(), None if fasta_first else bytes([GOOD]) * n)
    fl = {"fastq_150": 150, "fasta_k1": k + 1, "fasta_k": k, "fastq_k": k}[first]
    fs = rng.choice(np.frombuffer(b"ACGT", np.uint8), fl).tobytes()
    first_rec = (fs, None if fasta_first else bytes([GOOD]) * fl)
    recs = recs[:a] + [neighbour, first_rec] + recs[a:]
    return pack(recs), a + 1, a + 1 + 101


# ---------------------------------------------------------------- FASTA records on tile edges
def fa_tile_batch(k, lead, final_extra=0):
    """(batch, marks): FASTA-only records behind a leading record of `lead` bases (off[1] = lead);
    the tile arithmetic is that of the sub-range [1, n): t0 = off[1] & ~15, tiles of FA_TILE.
      record 1  spans three tiles; an N at t0 + FA_TILE j - 1, t0 + FA_TILE j and
                t0 + FA_TILE j - (k - 1) for j = 1, 2; its final N-free segment is k + final_extra
      record 2  filler up to 4 bytes before the third tile edge
      run       48 records of lengths 0 .. k + 2 (cycling): the first of them share one lane's 16
                starts with the filler's tail, and one lies across the tile edge
      last      a record with a NUL exactly on the fourth tile edge
    marks: t0, n_pos (the N positions of record 1), final_n, run (first, last + 1 record index),
    run_edge, nul_pos."""
    rng = np.random.default_rng([k, lead, final_extra])
    acgt = np.frombuffer(b"ACGT", np.uint8)
    t0 = lead & ~15
    T = FA_TILE
    recs = [(rng.choice(acgt, lead).tobytes(), None)]
    end1 = t0 + 2 * T + 300
    s = rng.choice(acgt, end1 - lead)
    n_pos = [t0 + T * j + d for j in (1, 2) for d in (-1, 0, -(k - 1))]
    final_n = end1 - (k + final_extra) - 1
    for p in n_pos + [final_n]:
        s[p - lead] = ord("N")
    recs.append((s.tobytes(), None))
    run_edge = t0 + 3 * T
    recs.append((rng.choice(acgt, run_edge - 4 - end1).tobytes(), None))
    run0 = len(recs)
    for i in range(48):
        recs.append((rng.choice(acgt, (i + 1) % (k + 3)).tobytes(), None))   # 1, 2, 3, ...
    pos = run_edge - 4 + sum(len(r[0]) for r in recs[run0:])
    nul_pos = t0 + 4 * T
    s = rng.choice(acgt, nul_pos - pos + 200)
    s[nul_pos - pos] = 0
    recs.append((s.tobytes(), None))
    marks = {"t0": t0, "n_pos": n_pos, "final_n": final_n, "run": (run0, run0 + 48),
             "run_edge": run_edge, "nul_pos": nul_pos}
    return pack(recs), marks


# ---------------------------------------------------------------- predicates (from off alone)
def wave_bases(off):
    """off[r0] of every wave of RK_READS reads."""
    n = len(off) - 1
    return np.asarray(off)[np.arange(0, n, RK_READS)]


def wave_spans(off):
    """k_rk_span: off[r1] - (off[r0] & ~15) per wave of RK_READS reads; a wave stages its bytes
    in LDS iff its span is <= RK_CAP."""
    off = np.asarray(off)
    n = len(off) - 1
    r0 = np.arange(0, n, RK_READS)
    r1 = np.minimum(n, r0 + RK_READS)
    return off[r1] - (off[r0] & ~np.int64(15))


def fa_tile_origin(off):
    """k_fa_kmers / k_sh1_nul: tile j starts at (off[0] & ~15) + FA_TILE j."""
    return int(off[0]) & ~15


def lanes_with_multiple_records(off, hasq):
    """Per k_fa_kmers lane (FA_CPT consecutive positions from fa_tile_origin), the number of
    non-empty records without qualities that hold one of its positions: each is one trip of the
    lane's record loop that may write keys."""
    off = np.asarray(off)
    t0 = fa_tile_origin(off)
    lanes = (int(off[-1]) - t0 + FA_CPT - 1) // FA_CPT
    cnt = np.zeros(max(lanes, 1), np.int64)
    for r in range(len(off) - 1):
        if hasq[r] or off[r + 1] == off[r]:
            continue
        cnt[(int(off[r]) - t0) // FA_CPT:(int(off[r + 1]) - 1 - t0) // FA_CPT + 1] += 1
    return cnt


# ---------------------------------------------------------------- expected keys per record
def canonical_at(seq: bytes, starts, k: int) -> np.ndarray:
    """fq_walk.canonical at every start, vectorised (tests/test_packed_inputs.py pins it to
    fq_walk.record_keys)."""
    starts = np.asarray(starts, np.int64)
    if not len(starts):
        return np.zeros(0, np.uint64)
    code = ((np.frombuffer(seq, np.uint8) >> 1) & 3).astype(np.uint64)
    c = code[starts[:, None] + np.arange(k)]
    j = np.arange(k, dtype=np.uint64)
    f = (c << (np.uint64(2) * (np.uint64(k - 1) - j))).sum(1, dtype=np.uint64)
    r = (((c + np.uint64(2)) & np.uint64(3)) << (np.uint64(2) * j)).sum(1, dtype=np.uint64)
    return np.minimum(f, r)


def sh1_keys(rec, k: int, min_quality: int = MQ) -> np.ndarray:
    """fq_walk.record_keys: fq_walk's classification and window walk, the keys vectorised."""
    s, q = rec
    cls = W.classify(s, q, W.threshold_char(min_quality))
    return canonical_at(s, W.window_starts(cls, k), k)


def rp_keys(rec, k: int, min_q: int = MQ_RP) -> np.ndarray:
    from oracle import oracle as O
    return O.read_kmers(rec[0], rec[1], k, min_q)


@functools.lru_cache(maxsize=None)
def record_keys_cached(walk: str, k: int, which: tuple):
    """Per-record expected keys of a generated batch, computed once: which = ("ragged", seed, n,
    share3) | ("sub", seed, variant) | ("fa", lead, final_extra)."""
    if which[0] == "ragged":
        recs = ragged_batch(which[1], k, which[2], which[3] / 3)[0]
    elif which[0] == "sub":
        recs = sub_range_batch(which[1], k, which[2])[0][0]
    else:
        recs = fa_tile_batch(k, which[1], which[2])[0][0]
    if walk == "rp_noq":
        recs = [(s, None) for s, _ in recs]
    f = sh1_keys if walk == "sh1" else rp_keys
    return [f(r, k) for r in recs]


def table_of_keys(per_record) -> tuple:
    """(keys ascending u64, counts i32): a Counter over the per-record expected keys."""
    c = Counter()
    for a in per_record:
        c.update(a.tolist())
    keys = np.array(sorted(c), np.uint64)
    return keys, np.array([c[int(x)] for x in keys], np.int32)
