"""The chain pass's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_chains.h (the parameter and block checks, the candidate predicate, the
cost, the key packing and the window search the kernels of kmhg_chains.hip evaluate) is driven by
tools/asan/chains_check, a stand-alone program built with ASan + UBSan: a host loop over the same
functions (keys, sort, windows, minima, links, pointer jumping, sums, compaction) against an
O(B^2) restatement of the definition in include/kmhgpu.h.  tests/chains_ref.py -- the numpy
restatement every GPU chains test checks against -- is pinned on literals here."""
import os
import subprocess

import numpy as np
import pytest

import chains_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "chains_check")
M = 2**31 - 1


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "chains_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, (args, r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return [l for l in r.stdout.split("\n") if l]


def test_crafted_block_sets_match_the_definition(exe):
    """The refusals and their words, the predicate at the max_dist and max_drift edges and at the
    extreme coordinates, the key order on ties, the window search; then empty, one block, the
    edges, overlaps, contests, ties, staircases up to 1,025 blocks, a fan of 300 candidates and
    the extremes, each at six max_dist, four max_drift and four min_hits."""
    got = run(exe, "crafted")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 40


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_block_sets_match_the_definition(exe, seed):
    # blocks inside the cells of grids of up to 15 x 15, at the low and the high end of the range
    assert run(exe, "random", seed, 100) == ["ok 100"]


def _c(blocks, *a):
    chains, member = chains_ref.chains(blocks, *a)
    assert chains.dtype == np.int32 and member.dtype == np.int32
    return chains.tolist(), member.tolist()


def test_chains_ref_literals():
    assert chains_ref.chains(np.zeros((0, 4), np.int32), 5, 5)[0].shape == (0, 6)
    assert chains_ref.chains(np.zeros((0, 4), np.int32), 5, 5)[1].shape == (0,)
    assert _c([(5, 9, 4, 3)], 0, 0) == ([[5, 9, 8, 12, 3, 1]], [1])
    # gi = gj = 3 and 4 at max_dist = 3
    assert _c([(1, 1, 4, 4), (8, 8, 2, 2)], 3, 0) == ([[1, 1, 9, 9, 6, 2]], [1, 1])
    assert _c([(1, 1, 4, 4), (9, 9, 2, 2)], 3, 0) == \
        ([[1, 1, 4, 4, 4, 1], [9, 9, 10, 10, 2, 1]], [1, 2])
    # a diagonal shift of 2 and of 3 at max_drift = 2
    assert _c([(1, 1, 4, 4), (6, 8, 2, 2)], 9, 2) == ([[1, 1, 7, 9, 6, 2]], [1, 1])
    assert _c([(1, 1, 4, 4), (6, 9, 2, 2)], 9, 2)[1] == [1, 2]
    # overlap by one row in i only, in j only
    assert _c([(1, 1, 4, 4), (4, 9, 2, 2)], 2**40, 2**40)[1] == [1, 2]
    assert _c([(1, 1, 4, 4), (9, 4, 2, 2)], 2**40, 2**40)[1] == [1, 2]
    # two successors, the nearer wins; the loser does not fall back
    assert _c([(1, 1, 4, 4), (6, 6, 2, 2), (7, 9, 1, 1)], 9, 9) == \
        ([[1, 1, 7, 7, 6, 2], [7, 9, 7, 9, 1, 1]], [1, 1, 2])
    # equal-cost predecessors, equal-cost successors: the lower index
    assert _c([(1, 3, 1, 1), (3, 1, 1, 1), (5, 5, 1, 1)], 9, 9) == \
        ([[1, 3, 5, 5, 2, 2], [3, 1, 3, 1, 1, 1]], [1, 2, 1])
    assert _c([(1, 1, 2, 2), (4, 6, 1, 1), (6, 4, 1, 1)], 9, 9) == \
        ([[1, 1, 4, 6, 3, 2], [6, 4, 6, 4, 1, 1]], [1, 1, 2])
    # min_hits drops the middle chain and renumbers the later one
    assert _c([(1, 1, 4, 4), (2, 50, 1, 1), (6, 6, 2, 2), (90, 90, 3, 3)], 9, 9, 2) == \
        ([[1, 1, 7, 7, 6, 2], [90, 90, 92, 92, 3, 1]], [1, 0, 1, 2])
    assert _c([(1, 1, 4, 4), (2, 50, 1, 1)], 9, 9, 2**40) == ([], [0, 0])
    # the extreme coordinates: gaps of M - 4
    ext = [(1, 1, 2, 2), (M - 1, M - 1, 2, 1)]
    assert _c(ext, M - 4, 0) == ([[1, 1, M, M, 3, 2]], [1, 1])
    assert _c(ext, M - 5, 0)[1] == [1, 2]
    for bad in ([(1, 2, 1, 1), (1, 2, 1, 1)], [(2, 1, 1, 1), (1, 9, 1, 1)], [(1, 1, 0, 1)],
                [(1, 1, 2, 3)], [(1, 1, 2, 0)], [(2, 1, M, 1)], [(0, 1, 1, 1)]):
        with pytest.raises(AssertionError):
            chains_ref.chains(bad, 5, 5)


def test_max_dist_zero_links_only_touching_blocks():
    rng = np.random.default_rng(5)
    for _ in range(20):
        cells = rng.integers(2, 12)
        keep = rng.random((cells, cells)) < rng.random()
        ci, cj = np.nonzero(keep)
        span = rng.integers(1, 5, len(ci))
        b = np.stack([1 + 6 * ci, 1 + 6 * cj + rng.integers(0, 2, len(ci)), span,
                      rng.integers(1, span + 1)], axis=1)          # gaps >= 1: nothing touches
        chains, member = chains_ref.chains(b, 0, 2**40)
        assert np.array_equal(chains, np.column_stack(
            [b[:, 0], b[:, 1], b[:, 0] + b[:, 2] - 1, b[:, 1] + b[:, 2] - 1, b[:, 3],
             np.ones(len(b), np.int64)]))
        assert np.array_equal(member, np.arange(1, len(b) + 1))
