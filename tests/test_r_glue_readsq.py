"""The R glue's reads_kmer_positions / reads_kmer_votes (reads.kmer.pos, reads.kmer.vote) over
tests/rshim (see tests/test_r_glue.py for the stand-in R runtime).  They are exported from the glue
but not in its registration table, so they are called by symbol.  error() outside a registered
call aborts the stand-in runtime after printing the message, so each refusal runs in a child
process of its own; every refusal of an argument is raised before the library is called, so no
such child touches the GPU (CPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from reads_ref import rows_ref, votes_ref
from test_r_glue import ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    r.L.reads_kmer_positions.restype = C.c_void_p
    r.L.reads_kmer_positions.argtypes = [C.c_void_p] * 4
    r.L.reads_kmer_votes.restype = C.c_void_p
    r.L.reads_kmer_votes.argtypes = [C.c_void_p] * 5
    yield r
    r.L.fr_reset()


def test_entry_points_exported_wrapped_and_not_registered(R):
    assert R.L.reads_kmer_positions and R.L.reads_kmer_votes
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    assert ('reads.kmer.pos <- function(ex.ptr, seqs, k, strand=0){ '
            'm <- .Call("reads_kmer_positions", ex.ptr, as.character(seqs), as.integer(k), '
            'as.integer(strand)) rownames(m) <- c("read", "strand", "i", "j") t(m) }') in txt
    assert ('reads.kmer.vote <- function(ex.ptr, seqs, k, band=64, strand=0){ '
            'm <- .Call("reads_kmer_votes", ex.ptr, as.character(seqs), as.integer(k), '
            'as.integer(band), as.integer(strand)) '
            'rownames(m) <- c("read", "strand", "pos", "hits", "second", "total") t(m) }') in txt
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert not {"reads_kmer_positions", "reads_kmer_votes"} & names
    assert "sequence_kmer_positions" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
p, v = R.L.reads_kmer_positions, R.L.reads_kmer_votes
p.restype, p.argtypes = C.c_void_p, [C.c_void_p] * 4
v.restype, v.argtypes = C.c_void_p, [C.c_void_p] * 5
args = dict(ptr=R.nil(), seqs=R.s("ACGTACGTAC", "ACGT"), k=R.i(5), band=R.i(64), strand=R.i(0))
args.update({name}={value})
if {votes}:
    v(args["ptr"], args["seqs"], args["k"], args["band"], args["strand"])
else:
    p(args["ptr"], args["seqs"], args["k"], args["strand"])
print("returned")
"""

K1 = "k should be an integer of length 1"
STRAND = "strand should be 0 (both), 1 (forward) or -1 (reverse)"
BAND1 = "band should be an integer of length 1"


@pytest.mark.parametrize("votes,name,value,message", [
    (False, "seqs", "R.i(1)", "seqs should be a character vector"),
    (False, "k", "R.d(5.0)", K1),
    (False, "k", "R.i(5, 6)", K1),
    (False, "k", "R.i(0)", "k should be between 1 and 31"),
    (False, "k", "R.i(32)", "k should be between 1 and 31"),
    (False, "strand", "R.d(1.0)", STRAND),
    (False, "strand", "R.i(2)", STRAND),
    (False, "strand", "R.i(-2**31)", STRAND),
    (False, "ptr", "R.nil()", "ptr_r should be an external pointer"),
    (True, "band", "R.d(64.0)", BAND1),
    (True, "band", "R.i(1, 2)", BAND1),
    (True, "band", "R.i(-2**31)", BAND1),
    (True, "band", "R.i(0)", "band must be between 1 and 2^30"),
    (True, "band", "R.i(2**30 + 1)", "band must be between 1 and 2^30"),
    (True, "k", "R.i(40)", "k should be between 1 and 31"),
    (True, "ptr", "R.nil()", "ptr_r should be an external pointer"),
])
def test_refusals_carry_their_words(votes, name, value, message):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD.format(here=HERE, root=ROOT, name=name, value=value, votes=votes)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert f"fake_r: error() outside a call: {message}\n" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_rows_and_votes_through_the_glue(gpu, R, testfa):
    s, k = testfa[:6000], 15
    reads = [s[100:250], s[3000:3100], "ACGT", "", "N" * 40, s[5000:5160].lower()]
    ptr = R.call("make_kmer_h_index", R.s(s), R.i(k), R.i(0))
    ox = O.OracleIndex(s, k)
    for strand, strands in ((0, 3), (1, 1), (-1, 2)):
        want = rows_ref(s, k, reads, k, strands, 0, ox)
        got = R.int_matrix(R.L.reads_kmer_positions(ptr, R.s(*reads), R.i(k), R.i(strand)))
        assert got.shape[1] == 4 and np.array_equal(got, want)
        v = R.int_matrix(R.L.reads_kmer_votes(ptr, R.s(*reads), R.i(k), R.i(7), R.i(strand)))
        assert np.array_equal(v, votes_ref(want, len(reads), k, 7))
    assert R.L.fr_finalize(ptr) == 1
