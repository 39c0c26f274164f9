"""The diagonal-segment pass's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_segs.h (the pairing key, the (i, j) compare and the galloping bounded
search the kernels of kmhg_segs.hip run per row) is driven by tools/asan/segs_check, a
stand-alone program built with ASan + UBSan: a host loop over the same functions (classify, pair
by std::sort, filter) against a std::set restatement of the definition in include/kmhgpu.h.
tests/segs_ref.py -- the numpy restatement every GPU segments test checks against -- is pinned on
literals and on the figures measured on the oracle's rows."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
import segs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "segs_check")


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "segs_check"],
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
    """Empty, one row, one diagonal and all-singles at the tile sizes, interleaved diagonals, full
    blocks, a period-4 repeat, the extreme coordinates (1 and 2^31 - 1 on either axis), the key
    round trip and order, and the two input faults."""
    got = run(exe, "crafted")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 40


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_row_sets_match_the_definition(exe, seed):
    # grids of up to 40 x 40 at 1 .. 100 % density, at the low and the high end of the coordinates
    assert run(exe, "random", seed, 3000) == ["ok 3000"]


def test_segs_ref_literals():
    assert segs_ref.segments(np.zeros((0, 2), np.int32)).shape == (0, 3)
    assert segs_ref.segments([(1, 1)]).tolist() == [[1, 1, 1]]
    rows = [(1, 1), (1, 3), (2, 2), (2, 4), (3, 1), (3, 3), (4, 4)]
    assert segs_ref.segments(rows).tolist() == [[1, 1, 4], [1, 3, 2], [3, 1, 1]]
    assert segs_ref.segments(rows, 2).tolist() == [[1, 1, 4], [1, 3, 2]]
    assert segs_ref.segments(rows, 5).shape == (0, 3)
    assert segs_ref.expand([[1, 3, 2], [1, 1, 4], [3, 1, 1]]).tolist() == [list(r) for r in rows]
    m = 2**31 - 1
    assert segs_ref.segments([(1, m - 1), (2, m), (m - 1, 1), (m, 2)]).tolist() == \
        [[1, m - 1, 2], [m - 1, 1, 2]]
    with pytest.raises(AssertionError):
        segs_ref.segments([(2, 2), (1, 1)])
    with pytest.raises(AssertionError):
        segs_ref.segments([(1, 1), (1, 1)])


def test_segs_ref_on_oracle_rows_gives_the_measured_figures(testfa):
    """test.fa[:6000], k = 15, self: 5,275,316 rows, which the run format leaves at 5,275,280
    runs, are 53,933 maximal diagonals, the longest 5,986 rows, 2,344 of one row; "ACGT" * 600 at
    k = 5: 1,435,204 rows, 1,197 diagonals."""
    s = testfa[:6000]
    rows = O.OracleIndex(s, 15).query(s, 15).reshape(-1, 2)
    g = segs_ref.segments(rows)
    assert (len(rows), len(g), int(g[:, 2].max()), int((g[:, 2] == 1).sum())) == \
        (5_275_316, 53_933, 5_986, 2_344)
    d = np.diff(rows.astype(np.int64), axis=0)
    assert 1 + int(((d[:, 0] != 1) | (d[:, 1] != 1)).sum()) == 5_275_280
    s = "ACGT" * 600
    rows = O.OracleIndex(s, 5).query(s, 5).reshape(-1, 2)
    assert (len(rows), len(segs_ref.segments(rows))) == (1_435_204, 1_197)
