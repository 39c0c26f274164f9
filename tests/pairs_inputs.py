"""The named inputs of the kmer.pairs tests, built once and used by test_pairs_ref.py (CPU: the two
restatements against each other, and every fact a case is built to have) and test_gpu_pairs.py
(the kernels against pairs_ref).

k_join_probe / k_join_emit (kmhg_join.hip) work on tiles of TILE keys of `a` in a's kmer.pos row
order, BLOCK threads each; a case puts something at an edge of that tiling.  An i.i.d. sequence at
k = 31 has every window a distinct k-mer, so a key's first-occurrence rank is its window's start;
test_pairs_ref.py asserts that for every case that leans on it."""
import functools
from typing import NamedTuple

import numpy as np

import pairs_ref as R
from kmer_hasher_amd import synth

TILE, BLOCK = 2048, 256
SIDE_KEY = 2**64 - 1                       # 32 x G: the table's side-slot key (EMPTY_KEY)
_BASES = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.zeros(256, np.uint8)
_CODE[list(b"ACGT")] = np.arange(4, dtype=np.uint8)


class Case(NamedTuple):
    a: bytes
    b: bytes
    k: int
    dirs: tuple = ("ab", "ba", "aa")       # which of (a, b), (b, a), (a, a) the tests run
    facts: dict = {}


def differ(s: np.ndarray, seed: int) -> np.ndarray:
    """Every base of `s` replaced by another one, which of the three drawn i.i.d."""
    return _BASES[(_CODE[s] + 1 + _CODE[synth.iid(s.size, seed)] % 3) % 4]


def _not(s: np.ndarray, at, base: int) -> None:
    for i in at:
        if 0 <= i < s.size and s[i] == base:
            s[i] = ord("C")


def _ua_edge(U: int) -> Case:
    a = synth.iid(31, 3).tobytes() + b"N" if U == 1 else synth.iid(U + 30, 1000 + U).tobytes()
    return Case(a, a, 31, ("ab",), {"U": U})


def _empty_middle_tile() -> Case:
    a = synth.iid(3 * TILE + 30, 21)
    b = a.copy()
    # every window starting in [TILE, 2 * TILE) holds a base of [TILE + 30, 2 * TILE); none other
    b[TILE + 30:2 * TILE] = differ(a[TILE + 30:2 * TILE], 22)
    return Case(a.tobytes(), b.tobytes(), 31, facts={"U": 3 * TILE})


def _holes() -> Case:
    k = 31
    U = 2 * TILE + 500
    a = synth.iid(U + k - 1, 23)
    b = a.copy()
    at = np.arange(17, a.size, 2 * k + 3)
    b[at] = differ(a[at], 24)              # k windows lost around each, k + 3 kept between two
    return Case(a.tobytes(), b.tobytes(), k, facts={"U": U})


def _heavy(rank: int) -> Case:
    """A's first window of the poly-A k-mer starts at 0-based `rank`: 300 of it in a, 299 in b."""
    k, na = 31, 300
    run = na + k - 1
    s = synth.iid(rank + run + 700, 25 + rank).copy()
    s[rank:rank + run] = ord("A")
    _not(s, (rank - 1, rank + run), ord("A"))
    a = s.tobytes()
    b = a[:rank] + a[rank + 1:]
    return Case(a, b, k, facts={"rank": rank, "count_a": na, "count_b": na - 1,
                                "key": 0})   # 31 x A


def _inline_list_mix() -> Case:
    k = 31
    s = synth.iid(k * 10, 27).tobytes()
    K = [s[k * i:k * (i + 1)] for i in range(10)]
    #            (na, nb): K0 (1, 1)  K1 (1, 3)  K2 (2, 1)  K3 (3, 2)  K4 (1, 0)  K5 (2, 0)
    #                      K6 (1, 5000)  K7 (5000, 1); K8, K9 in b only
    a = K[:8] + [K[2], K[3], K[3], K[5]] + [K[7]] * 4999
    b = [K[0], K[8], K[1], K[1], K[1], K[2], K[3], K[9], K[3]] + [K[6]] * 5000 + [K[7]]
    want = [(1, 1), (1, 3), (2, 1), (3, 2), (1, 0), (2, 0), (1, 5000), (5000, 1)]
    # (an N after the last piece too: the window rule drops the first window after an N when it
    # ends with the string; (a, a) would be 5000^2 rows of one key, which no test here needs)
    return Case(b"N".join(a) + b"N", b"N".join(b) + b"N", k, ("ab", "ba"), {"counts": want})


def _geometry() -> Case:
    big = synth.iid(400_000, 29).tobytes()
    return Case(big[123_457:123_657], big, 31, ("ab", "ba"))


def _side_slot(which: str) -> Case:
    """k = 32: 16 windows of 32 x G in a (a run of 47), 27 in b (a run of 58), or in one only."""
    s = synth.iid(3000, 31).copy()
    _not(s, (699, 700, 999, 1000), ord("G"))
    plain = s.tobytes()
    a = plain[:1000] + b"G" * 47 + plain[1000:] if which != "b_only" else plain
    b = plain[:700] + b"G" * 58 + plain[700:] if which != "a_only" else plain
    return Case(a, b, 32, facts={"side_a": 16 if which != "b_only" else 0,
                                 "side_b": 27 if which != "a_only" else 0})


def _n_and_case() -> Case:
    k = 9
    base = synth.iid(6000, 37)
    a = synth.add_lowercase(base, 0.3, 5).copy()
    a[50:53] = ord("N")                    # then 9 = k bases (one window), N, 8 = k - 1 bases, N
    a[62] = a[71] = ord("n")
    a[2000:2100] = ord("N")
    b = base.copy()
    at = np.arange(40, b.size, 97)
    b[at] = differ(base[at], 38)
    b[10:14] = ord("N")
    b[3000:3050] = ord("n")
    b[4000] = b[4010] = b[4019] = ord("N")  # 9 bases, then 8, between them
    return Case(a.tobytes(), b.tobytes(), k,
                facts={"lone_a": 54, "none_a": (43, 73), "lone_b": 4002, "none_b": (3993, 4021)})


def _empty(which: str) -> Case:
    b = synth.iid(3000, 41).tobytes()
    a = b"N" * 100 if which == "all_n" else synth.iid(500, 43).tobytes()
    return Case(a, b, 31, ("ab", "ba"))


def _khash() -> Case:
    s = synth.iid(4500, 57)
    a = np.concatenate([s, s[:1000]])
    b = a.copy()
    at = np.arange(25, b.size, 50)
    b[at] = differ(a[at], 58)
    return Case(a.tobytes(), b.tobytes(), 11, ("ab",))


UA_EDGES = (1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7)
HEAVY_RANKS = (TILE - 1, TILE, 0)
SHORT_A = (synth.iid(31, 45).tobytes(), 31)         # length k: no build takes it

_MAKERS = {
    **{f"ua_{U}": functools.partial(_ua_edge, U) for U in UA_EDGES},
    "empty_middle_tile": _empty_middle_tile,
    "holes": _holes,
    **{f"heavy_rank_{r}": functools.partial(_heavy, r) for r in HEAVY_RANKS},
    "inline_list_mix": _inline_list_mix,
    "geometry": _geometry,
    **{f"side_{w}": functools.partial(_side_slot, w) for w in ("both", "a_only", "b_only")},
    "n_and_case": _n_and_case,
    "empty_all_n": functools.partial(_empty, "all_n"),
    "empty_disjoint": functools.partial(_empty, "disjoint"),
    "khash": _khash,
}
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return _MAKERS[name]()


RUNS = tuple((n, d) for n in NAMES for d in case(n).dirs)


def sides(name: str, d: str) -> tuple:
    c = case(name)
    return {"ab": (c.a, c.b), "ba": (c.b, c.a), "aa": (c.a, c.a)}[d]


@functools.lru_cache(maxsize=None)
def want(name: str, d: str) -> np.ndarray:
    """pairs_ref of one direction of a case, computed once; read-only."""
    x, y = sides(name, d)
    w = R.pairs_ref(x, y, case(name).k)
    w.setflags(write=False)
    return w


# ---- counts indices (count.kmers): specs {name: (k, source_n, calls)} and the pairings run
@functools.lru_cache(maxsize=None)
def count_specs() -> dict:
    k = 9
    x1 = synth.iid(5000, 51)
    x2 = x1.copy()
    at = np.arange(7, x2.size, 40)
    x2[at] = differ(x1[at], 52)
    x1, x2 = x1.tobytes(), x2[300:].tobytes()
    x3 = synth.iid(3000, 53).tobytes() + x1[:1000]
    return {
        "pos1": (k, 0, x1),                 # source_n 0: a position index of the sequence
        "pos2": (k, 0, x2),
        "c1_single": (k, 1, [(0, [x1])]),
        "c1_multi": (k, 1, [(0, [x1]), (0, [x2, b"ACGT"]), (0, [x1])]),   # known keys re-counted
        "c3_single": (k, 3, [(1, [x2])]),
        "c3_multi": (k, 3, [(0, [x1, x2]), (1, [x2]), (2, [x3]), (0, [x3])]),
    }


COUNT_RUNS = (
    ("c1_multi", "c3_multi"), ("c3_multi", "c1_single"), ("c1_single", "c1_multi"),
    ("c3_single", "c3_multi"), ("c3_multi", "c3_multi"),               # counts x counts
    ("pos1", "c1_multi"), ("pos2", "c3_multi"), ("pos1", "c3_single"),  # position x counts
    ("c1_multi", "pos2"), ("c3_multi", "pos1"), ("c1_single", "pos2"),  # counts x position
)


@functools.lru_cache(maxsize=None)
def count_table(name: str) -> dict:
    k, S, x = count_specs()[name]
    return R.kmer_starts(x, k) if S == 0 else R.kmer_counts(x, k, S)


@functools.lru_cache(maxsize=None)
def count_want(na: str, nb: str) -> np.ndarray:
    w = R.cross(count_table(na), count_table(nb))
    w.setflags(write=False)
    return w
