"""The block pass's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_blocks.h (the same-diagonal test, the gap, the span and the head
predicate the kernels of kmhg_blocks.hip evaluate per segment) is driven by tools/asan/blocks_check,
a stand-alone program built with ASan + UBSan: a host loop over the same functions (the segment
pass's front half, filter, heads, prefixes, the slot array) against a restatement of the
definition in include/kmhgpu.h that walks every diagonal of a std::map.  tests/blocks_ref.py --
the numpy restatement every GPU blocks test checks against -- is pinned on literals and on the
figures it gives on the oracle's rows."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
import blocks_ref
import segs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "blocks_check")
M = 2**31 - 1

# (max_gap, min_len, min_hits) -> (blocks, longest span, sum of hits, largest span - hits) of
# test.fa[:6000], k = 15, self (5,275,316 rows, 53,933 segments); tests/test_gpu_blocks.py
# asserts the device's result against the same figures
TESTFA_FIGURES = {
    (0, 1, 1): (53_933, 5_986, 5_275_316, 0),
    (15, 1, 1): (53_911, 5_986, 5_275_316, 15),
    (15, 2, 1): (51_567, 5_986, 5_272_972, 15),
    (15, 1, 100): (9_753, 5_986, 3_876_008, 0),
    (2**40, 1, 1): (10_871, 5_986, 5_275_316, 3_418),
}


def figures(b):
    return (len(b), int(b[:, 2].max()), int(b[:, 3].sum()), int((b[:, 2] - b[:, 3]).max()))


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "blocks_check"],
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


def test_crafted_row_sets_match_the_definition(exe):
    """Empty, one row, singles on one and on two interleaved diagonals at the tile sizes,
    alternating gaps, dropped segments that are bridged or open the gap, the extreme coordinates,
    each at min_len 1, 2, 3, 2^31, seven max_gap from 0 to 2^40 and min_hits 1, 2, 5, 2^31."""
    got = run(exe, "crafted")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 50


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_row_sets_match_the_definition(exe, seed):
    # grids of up to 40 x 40 at 1 .. 100 % density, at the low and the high end of the coordinates
    assert run(exe, "random", seed, 300) == ["ok 300"]


def _rows(segs):
    return segs_ref.expand(segs)


def test_blocks_ref_literals():
    assert blocks_ref.blocks(np.zeros((0, 2), np.int32), 5).shape == (0, 4)
    assert blocks_ref.blocks([(1, 1)], 0).tolist() == [[1, 1, 1, 1]]
    # two diagonals: d = 0 holds (1, 1, 3), (5, 5, 1), (7, 7, 2) with gaps 1 and 1; d = 7 holds
    # (2, 9, 2), (6, 13, 4) with gap 2
    rows = _rows([(1, 1, 3), (5, 5, 1), (7, 7, 2), (2, 9, 2), (6, 13, 4)])
    assert blocks_ref.blocks(rows, 0).tolist() == \
        [[1, 1, 3, 3], [2, 9, 2, 2], [5, 5, 1, 1], [6, 13, 4, 4], [7, 7, 2, 2]]   # max_gap = 0
    g = segs_ref.segments(rows)
    assert np.array_equal(blocks_ref.blocks(rows, 0), np.column_stack([g, g[:, 2]]))
    assert blocks_ref.blocks(rows, 1).tolist() == [[1, 1, 8, 6], [2, 9, 2, 2], [6, 13, 4, 4]]
    assert blocks_ref.blocks(rows, 2).tolist() == [[1, 1, 8, 6], [2, 9, 8, 6]]
    # min_len = 2 drops (5, 5, 1): the gap between its neighbours is 7 - 4 = 3 and spans it
    assert blocks_ref.blocks(rows, 3, 2).tolist() == [[1, 1, 8, 5], [2, 9, 8, 6]]     # bridged
    assert blocks_ref.blocks(rows, 2, 2).tolist() == [[1, 1, 3, 3], [2, 9, 8, 6], [7, 7, 2, 2]]
    assert blocks_ref.blocks(rows, 1, 2).tolist() == \
        [[1, 1, 3, 3], [2, 9, 2, 2], [6, 13, 4, 4], [7, 7, 2, 2]]
    assert blocks_ref.blocks(rows, 1, 1, 3).tolist() == [[1, 1, 8, 6], [6, 13, 4, 4]]   # min_hits
    assert blocks_ref.blocks(rows, 2**40, 1, 7).shape == (0, 4)
    assert blocks_ref.blocks(rows, 2**40, 5).shape == (0, 4)
    # the extreme coordinates: a gap of M - 4
    ext = [(1, 1), (2, 2), (M - 1, M - 1), (M, M)]
    assert blocks_ref.blocks(ext, M - 5).tolist() == [[1, 1, 2, 2], [M - 1, M - 1, 2, 2]]
    assert blocks_ref.blocks(ext, M - 4).tolist() == [[1, 1, M, 4]]
    assert blocks_ref.blocks(ext, M - 2).tolist() == [[1, 1, M, 4]]
    assert blocks_ref.merge([(M - 1, M - 1, 2), (1, 1, 2)], M - 4).tolist() == [[1, 1, M, 4]]
    with pytest.raises(AssertionError):
        blocks_ref.merge([(1, 1, 3), (3, 3, 2)], 0)          # overlapping: not maximal segments


def test_raising_max_gap_only_unions_blocks():
    rng = np.random.default_rng(11)
    for _ in range(50):
        keep = rng.random((30, 30)) < rng.random()
        rows = np.argwhere(keep) + 1
        prev = None
        for gap in (0, 1, 2, 3, 5, 9, M):
            b = blocks_ref.blocks(rows, gap).astype(np.int64)
            assert b[:, 3].sum() == len(rows)
            if prev is not None:                 # every earlier block lies inside one of these
                assert len(b) <= len(prev)
                for i, j, span, _ in prev:
                    inside = (b[:, 1] - b[:, 0] == j - i) & (b[:, 0] <= i) & \
                        (i + span <= b[:, 0] + b[:, 2])
                    assert inside.sum() == 1
            prev = b
        per_diag = len(np.unique(rows[:, 1] - rows[:, 0])) if len(rows) else 0
        assert len(prev) == per_diag             # max_gap >= 2^31 - 2: one block per diagonal


def test_blocks_ref_on_oracle_rows_gives_the_pinned_figures(testfa):
    s = testfa[:6000]
    rows = O.OracleIndex(s, 15).query(s, 15).reshape(-1, 2)
    for (max_gap, min_len, min_hits), want in TESTFA_FIGURES.items():
        assert figures(blocks_ref.blocks(rows, max_gap, min_len, min_hits)) == want, \
            (max_gap, min_len, min_hits)
