"""seq.kmer.raster's host-testable pieces, on the CPU.

kmer_hasher_amd/csrc/kmhg_raster.h (the frame checks with their words, the overflow rule, the
multiply-shift divisor constants, the cell index the kernels of kmhg_raster.hip evaluate per row
and the i-cell span of a tile) is driven by tools/asan/raster_check, a stand-alone program built
with ASan + UBSan.  tests/raster_ref.py -- the numpy restatement every GPU raster test checks
against -- is pinned on literals and on the properties of the definition in include/kmhgpu.h."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
import raster_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "tools", "asan", "raster_check")
M = 2**31 - 1


@pytest.fixture(scope="module")
def exe():
    # flock: pytest-xdist workers each run this fixture; one make at a time
    r = subprocess.run(["flock", os.path.join(ROOT, "tools", "asan", ".build.lock"),
                        "make", "-s", "-C", os.path.join(ROOT, "tools", "asan"), "raster_check"],
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


def test_frame_refusals_and_overflow_rule(exe):
    """Every refusal in its order and words with int64 extremes in the frame, the legal edge
    frames (width 1, width 2^31 - 1, coordinate 2^31 - 1, 2^26 cells), the overflow rule."""
    got = run(exe, "frames")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 30


def test_divisor_constants_equal_plain_division(exe):
    """d in [1, 4096], around every power of two, 2,000 random d up to 2^31 - 1; x near 0, near
    2^31 - 1, around multiples of d and at random; d <= 300 against every x below 70,000."""
    got = run(exe, "divisors")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 20_000_000


def test_cell_index_matches_the_definition(exe):
    got = run(exe, "cells")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 100_000


def test_tile_span_bound(exe):
    got = run(exe, "span")
    assert len(got) == 1 and got[0].startswith("ok ") and int(got[0][3:]) >= 10_000


# ------------------------------------------------------------------ raster_ref itself
def test_raster_ref_literals():
    rows = [(1, 1), (2, 2), (2, 3), (5, 9), (6, 1), (0, 1), (1, 0), (-4, 2)]
    assert raster_ref.raster(rows, (1, 1, 2, 4, 3, 3)).tolist() == [[3, 0, 0], [0, 0, 0], [1, 0, 1]]
    assert raster_ref.raster(rows, (2, 2, 1, 1, 1, 2)).tolist() == [[1, 1]]
    assert raster_ref.raster(rows, (1, 1, M, M, 1, 1)).tolist() == [[5]]
    assert raster_ref.raster(rows, (7, 1, 1, 1, 2, 2)).tolist() == [[0, 0], [0, 0]]
    assert raster_ref.raster(np.zeros((0, 2)), (1, 1, 1, 1, 2, 1)).tolist() == [[0], [0]]
    assert raster_ref.raster([(M, M), (M, 1)], (M, M, 1, 1, 1, 1)).tolist() == [[1]]
    assert raster_ref.window_counts(10, 1, 4, 3).tolist() == [4, 4, 2]
    assert raster_ref.window_counts(10, 3, 4, 3).tolist() == [4, 4, 0]


@pytest.fixture(scope="module")
def rows(testfa):
    s = testfa[:1500]
    return O.OracleIndex(s, 15).query(s, 15).reshape(-1, 2)


FRAMES = [(1, 1, 1, 1, 1500, 1500), (1, 1, 3, 5, 500, 300), (200, 100, 2, 2, 300, 400),
          (1, 1000, 7, 1, 100, 600), (1, 1, 2**20, 2**20, 1, 1), (1400, 1400, 1, 1, 500, 500)]


@pytest.mark.parametrize("frame", FRAMES)
def test_sum_is_the_in_frame_row_count(rows, frame):
    m = raster_ref.raster(rows, frame)
    assert m.shape == (frame[4], frame[5]) and (m >= 0).all()
    assert int(m.sum()) == raster_ref.in_frame(rows, frame)
    i_lo, j_lo, bin_i, bin_j, n_i, n_j = frame
    slow = sum(1 for i, j in rows.tolist()
               if i_lo <= i < i_lo + n_i * bin_i and j_lo <= j < j_lo + n_j * bin_j)
    assert int(m.sum()) == slow
    assert (m <= bin_i * bin_j).all()                # rows are distinct


def test_width_one_bins_reproduce_the_rows(rows):
    for i_lo, j_lo, n_i, n_j in ((1, 1, 1500, 1500), (300, 200, 700, 900)):
        m = raster_ref.raster(rows, (i_lo, j_lo, 1, 1, n_i, n_j))
        assert set(np.unique(m).tolist()) <= {0, 1}
        bi, bj = np.nonzero(m)
        back = np.stack([bi + i_lo, bj + j_lo], axis=1)
        inside = rows[(rows[:, 0] >= i_lo) & (rows[:, 0] < i_lo + n_i) &
                      (rows[:, 1] >= j_lo) & (rows[:, 1] < j_lo + n_j)]
        assert np.array_equal(back, inside)          # both ascending by (i, j)


@pytest.mark.parametrize("fi,fj", [(1, 1), (2, 2), (3, 7), (10, 1), (64, 64), (2000, 3)])
def test_coarsening_equals_the_coarser_frame(rows, fi, fj):
    for i_lo, j_lo, bin_i, bin_j, n_i, n_j in ((1, 1, 1, 1, 1500, 1500), (50, 9, 2, 3, 601, 403)):
        fine = raster_ref.raster(rows, (i_lo, j_lo, bin_i, bin_j, n_i, n_j))
        cn_i, cn_j = -(-n_i // fi), -(-n_j // fj)
        coarse = raster_ref.raster(rows, (i_lo, j_lo, bin_i * fi, bin_j * fj, cn_i, cn_j))
        # the coarser frame reaches past the finer one's last cells; cut it back to compare
        keep = rows[(rows[:, 0] < i_lo + n_i * bin_i) & (rows[:, 1] < j_lo + n_j * bin_j)]
        coarse_cut = raster_ref.raster(keep, (i_lo, j_lo, bin_i * fi, bin_j * fj, cn_i, cn_j))
        assert np.array_equal(raster_ref.coarsen(fine, fi, fj), coarse_cut)
        assert (coarse >= coarse_cut).all()
