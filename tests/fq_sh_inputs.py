"""Inputs of the count.kmers.fq.sh / kmer.spec.sh tests: the reference's own fixtures with
test.R's parameter shapes, and seeded edge records for the two kernels.  Deterministic; shared by
tests/golden/make_fq_sh_golden.py and the tests.

Qualities of the seeded records: with min_quality = 30 the threshold char is '?'; 'I' is good,
'?' weak, '#' bad.  params = (k, report_n, prefix_bits, max_memory, min_quality, max_read_n).
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FA_TILE = 4096          # k_fa_kmers: window starts (chars) per workgroup (kmhg_sh.h FA_TILE)
LANE_KS = (5, 9, 20, 21, 31)
FA_KS = (9, 20, 21)
GOOD, WEAK, BAD = ord("I"), ord("?"), ord("#")
MQ = 30


def prefix_bits_for(k: int) -> int:
    return max(min(20, 2 * k), 2 * k - 32)      # suffix bits 2k - prefix stay within 0 .. 32


def params(k, min_quality=MQ, max_read_n=-1, report_n=1, max_memory=100):
    return [k, report_n, prefix_bits_for(k), max_memory, min_quality, max_read_n]


# the reference's fixtures with test.R's parameter shapes (test.R:424-449), max_read_n 0 / 5 / -1,
# and two calls accumulated into one pointer: name -> [(file, params), ...]
FILE_CASES = {
    "repeat40_shape1": [("repeat_40.fq", [20, 1, 20, 100, 30, 100])],
    "repeat40_shape2": [("repeat_40.fq", [21, 100000, 18, 300, 30, 1000000])],
    "test10_shape1": [("test_10.fastq", [20, 1, 20, 100, 30, 100])],
    "test10_shape2_all": [("test_10.fastq", [21, 100000, 18, 300, 30, -1])],
    "test10_first5": [("test_10.fastq", [20, 1, 20, 100, 30, 5])],
    "test10_none": [("test_10.fastq", [20, 1, 20, 100, 30, 0])],
    "testgz_shape1": [("test.fastq.gz", [20, 1, 20, 100, 30, 100])],
    "testgz_shape2": [("test.fastq.gz", [21, 100000, 18, 300, 30, 1000000])],
    "testgz_q0_k31": [("test.fastq.gz", [31, 1, 30, 100, 0, -1])],
    "two_calls": [("test_10.fastq", [20, 1, 20, 100, 30, -1]),
                  ("repeat_40.fq", [20, 1, 20, 100, 10, -1])],
    "testfa_k20": [("test.fa", [20, 1, 20, 300, 30, -1])],
}
SPECTRA = (1, 3, 1000)      # below / around / above the largest counts of these inputs


def _bases(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n)


def _rec(rng, n, marks=()):
    """A record of n random bases, all good, then (position, quality) marks applied."""
    s = _bases(rng, n)
    q = np.full(n, GOOD, np.uint8)
    for p, v in marks:
        q[p] = v
    return s.tobytes(), q.tobytes()


def lane_cases(k: int) -> dict:
    """name -> (records [(seq, qual)], min_quality): the edge list of the lane-per-read walk."""
    rng = np.random.default_rng(1000 + k)
    n = 3 * k + 5
    c = {}
    c["short"] = ([_rec(rng, k - 1), _rec(rng, k), _rec(rng, k + 1), _rec(rng, n)], MQ)
    c["weak_first"] = ([_rec(rng, n, [(0, WEAK)])], MQ)
    c["weak_in_init"] = ([_rec(rng, n, [(k // 2, WEAK)])], MQ)
    c["weak_first_rolled"] = ([_rec(rng, n, [(k, WEAK)])], MQ)
    c["weak_last"] = ([_rec(rng, n, [(n - 1, WEAK)])], MQ)
    c["weak_km1_apart"] = ([_rec(rng, n, [(k + 2, WEAK), (2 * k + 1, WEAK)])], MQ)
    c["weak_k_apart"] = ([_rec(rng, n, [(k + 2, WEAK), (2 * k + 2, WEAK)])], MQ)
    c["bad_before_weak"] = ([_rec(rng, n, [(k + 1, BAD), (k + 2, WEAK)])], MQ)
    c["bad_after_weak"] = ([_rec(rng, n, [(k + 2, WEAK), (k + 3, BAD)])], MQ)
    bang = _rec(rng, n, [(3, ord("!")), (k + 4, ord("!")), (n - 1, ord("!"))])
    c["min_quality_0"] = ([bang, _rec(rng, n)], 0)
    c["final_segment_k"] = ([_rec(rng, n, [(n - k - 1, BAD)])], MQ)
    c["final_segment_k_then_bad"] = ([_rec(rng, n + 1, [(n - k - 1, BAD), (n, BAD)])], MQ)

    def mixed(count, length):
        out = []
        for _ in range(count):
            s = _bases(rng, length)
            s[rng.random(length) < 0.02] = ord("N")
            q = rng.choice(np.array([GOOD, WEAK, BAD], np.uint8), length, p=[.9, .06, .04])
            out.append((s.tobytes(), q.tobytes()))
        return out
    c["reads_64"] = (mixed(64, n + 7), MQ)
    c["reads_65"] = (mixed(65, n + 7), MQ)
    # 64 reads x 1000 bases: more than the 28 KiB a wave stages -> the global-memory cursor
    c["over_lds_cap"] = (mixed(64, 1000), MQ)
    return c


def fa_cases(k: int) -> dict:
    """name -> records [(seq, None)]: the edge list of the position-parallel kernel."""
    rng = np.random.default_rng(2000 + k)
    T = FA_TILE
    c = {}
    for L in (T - 1, T, T + 1, T + k - 1, 2 * T + 3):
        base = _bases(rng, L)
        marks = {"plain": [], "tile_last": [(T - 1, "N")], "tile_first": [(T, "n")],
                 "km1_before_edge": [(T - (k - 1), "N")],
                 "final_k": [(L - k - 1, "n")], "final_k1": [(L - k - 2, "N")]}
        for name, mk in marks.items():
            s = base.copy()
            for p, ch in mk:
                if 0 <= p < L:
                    s[p] = ord(ch)
            c[f"L{L}_{name}"] = [(s.tobytes(), None)]
    c["all_n"] = [(b"N" * (T + 5), None)]
    a = _bases(rng, T - 3).tobytes()
    c["two_records"] = [(a, None), (a[-(k - 1):] + _bases(rng, 2 * k).tobytes(), None)]
    return c


def fastx_bytes(records) -> bytes:
    out = []
    for i, (s, q) in enumerate(records):
        out.append(b">r%d\n%s\n" % (i, s) if q is None else b"@r%d\n%s\n+\n%s\n" % (i, s, q))
    return b"".join(out)


def golden_path() -> str:
    return os.path.join(GOLDEN, "fq_sh_golden.json")


def load_golden():
    with open(golden_path()) as f:
        return json.load(f)
