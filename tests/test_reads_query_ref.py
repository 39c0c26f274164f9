"""tests/reads_ref.py -- the checker of the GPU tests of reads.kmer.pos / reads.kmer.vote -- pinned
on the CPU: its forward rows against the compiled reference's seq_kmer_positions read by read on
the reference's own files, its vote against hand-computed cases."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from reads_ref import pack, rows_ref, votes_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def test_forward_rows_are_the_references_read_by_read(testfa):
    """The first 200 reads of test.fastq.gz against an index of test.fa at k = 15."""
    if not O.ref_available():
        pytest.skip("reference build not available")
    recs = O.fastx_records(O.read_fastx(os.path.join(HERE, "golden", "test.fastq.gz")))
    reads = [s.decode() for s, _ in recs][:200]
    assert len(reads) == 200
    k = 15
    got = rows_ref(testfa, k, reads, k, strands=1)
    ref = O.RefIndex(testfa, k)
    want = []
    for r, read in enumerate(reads, 1):
        if len(read) <= k:
            continue
        ij = np.asarray(ref.query(read, k), np.int32).reshape(-1, 2)
        want.append(np.column_stack([np.full(len(ij), r, np.int32), np.ones(len(ij), np.int32), ij]))
    ref.close()
    want = np.concatenate(want).astype(np.int32)
    assert want.shape[0] > 0 and np.array_equal(got, want)
    both = rows_ref(testfa, k, reads, k)
    assert np.array_equal(both[both[:, 1] == 1], want)
    assert (np.diff(both[:, 0]) >= 0).all()


def test_short_and_empty_reads_have_no_rows():
    a = "ACGTTGCAACGTNACGTAAAATTTT"
    assert rows_ref(a, 3, ["", "A", "ACG", "NNNN"], 3).shape == (0, 4)
    r = rows_ref(a, 3, ["ACG", "ACGT"], 3)
    assert r.shape[0] > 0 and set(r[:, 0].tolist()) == {2}


def test_pack():
    seq, off = pack(["AC", "", b"GTN"])
    assert seq.tobytes() == b"ACGTN" and off.tolist() == [0, 2, 2, 5]


def test_votes_hand_computed_ties():
    k = 3
    # read 1: 2 votes forward at pos 10, 2 votes reverse at pos 10 -> the strand tie goes forward;
    # read 2: 2 votes in bin 0 and 2 in bin 2 on the reverse strand -> the smaller bin; read 3: none
    rows = np.array([[1, 1, 4, 11], [1, 1, 5, 12], [1, -1, 4, 11], [1, -1, 6, 13],
                     [2, -1, 4, 2], [2, -1, 5, 3], [2, -1, 4, 18], [2, -1, 5, 19], [2, 1, 9, 40]],
                    np.int32)
    got = votes_ref(rows, 3, k, 8)
    assert got.tolist() == [[1, 1, 8, 2, 2, 4], [2, -1, 0, 2, 2, 5], [3, 0, 0, 0, 0, 0]]
    assert got.dtype == np.int32
    assert np.array_equal(votes_ref(rows[::-1], 3, k, 8), got)     # any row order


def test_votes_floor_for_negative_pos():
    k = 3
    # pos = j - i + k = -1, -7, -8 at band 7: bins -1, -1, -2 (truncation would give 0, -1, -1)
    rows = np.array([[1, 1, 5, 1], [1, 1, 11, 1], [1, 1, 12, 1]], np.int32)
    assert votes_ref(rows, 1, k, 7).tolist() == [[1, 1, -7, 2, 1, 3]]
    assert votes_ref(rows[2:], 1, k, 7).tolist() == [[1, 1, -14, 1, 0, 1]]
