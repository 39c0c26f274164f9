"""The R glue's sequence_kmer_chains (seq.kmer.chains) over tests/rshim (see tests/test_r_glue.py
for the stand-in R runtime).  Like sequence_kmer_blocks it is exported from the glue but not in
its registration table, so it is called by symbol.  error() outside a registered call aborts the
stand-in runtime after printing the message, so each refusal runs in a child process of its own
and is read from there; the argument checks come before any device work (CPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import blocks_ref
import chains_ref
from test_r_glue import INTSXP, ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))
VECSXP = 19


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    f = r.L.sequence_kmer_chains
    f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 10
    yield r
    r.L.fr_reset()


def test_entry_point_exported_wrapped_and_not_registered(R):
    assert R.L.sequence_kmer_chains
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    # the defaults (minimap2's -g and -r; max.gap = k as seq.kmer.blocks), the argument order of
    # the .Call, the column names and the list's names
    assert ('seq.kmer.chains <- function(ex.ptr, seq, k, max.dist=5000, max.drift=500, max.gap=k, '
            'min.len=1, min.hits=1, rc=FALSE, row.free=FALSE){') in txt
    assert ('r <- .Call("sequence_kmer_chains", ex.ptr, as.character(seq), as.integer(k), '
            'as.integer(max.dist), as.integer(max.drift), as.integer(max.gap), '
            'as.integer(min.len), as.integer(min.hits), as.integer(rc), as.integer(row.free)) '
            'rownames(r$chains) <- c("i", "j", "i.end", "j.end", "hits", "blocks") '
            'rownames(r$blocks) <- c("i", "j", "span", "hits") '
            'list(chains=t(r$chains), blocks=t(r$blocks), chain=r$chain) }') in txt
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert "sequence_kmer_chains" not in names and "sequence_kmer_positions" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
f = R.L.sequence_kmer_chains
f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 10
args = dict(ptr=R.nil(), seq=R.s("ACGTACGT"), k=R.i(3), max_dist=R.i(5000), max_drift=R.i(500),
            max_gap=R.i(3), min_len=R.i(1), min_hits=R.i(1), rc=R.i(0), row_free=R.i(0))
args.update({name}={value})
f(args["ptr"], args["seq"], args["k"], args["max_dist"], args["max_drift"], args["max_gap"],
  args["min_len"], args["min_hits"], args["rc"], args["row_free"])
print("returned")
"""


@pytest.mark.parametrize("name,value,message", [
    ("seq", 'R.s("ACGT", "ACGT")', "seq_r should be a single sequence"),
    ("k", "R.d(3.0)", "k should be an integer of length 1"),
    ("min_len", "R.i(0)", "min_len must be a positive integer"),
    ("max_gap", "R.i(-1)", "max_gap must not be negative"),
    ("max_dist", "R.i(-1)", "max_dist must not be negative"),
    ("max_dist", "R.d(5000.0)", "max_dist must not be negative"),
    ("max_drift", "R.i(-1)", "max_drift must not be negative"),
    ("max_drift", "R.i(1, 2)", "max_drift must not be negative"),
    ("min_hits", "R.i(0)", "min_hits must be a positive integer"),
    ("rc", "R.nil()", "rc should be an integer of length 1"),
    ("row_free", "R.nil()", "row_free should be an integer of length 1"),
    ("ptr", "R.nil()", "ptr_r should be an external pointer"),      # after the argument checks
    ("ptr", 'R.L.fr_extptr(None, b"other_tag")', "External pointer has incorrect tag"),
])
def test_refusals_carry_their_words(R, name, value, message):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD.format(here=HERE, root=ROOT, name=name, value=value)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert f"fake_r: error() outside a call: {message}\n" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_list_names_shapes_values_strands_and_routes(gpu, R, testfa):
    k = 15
    s = testfa[:1500]
    a = s[:700] + rc_host(s[700:1100]) + s[1100:]            # one inverted stretch
    ptr = R.call("make_kmer_h_index", R.s(a), R.i(k), R.i(0))
    oi = O.OracleIndex(a, k)
    for rc in (0, 1):
        rows = oi.query(rc_host(s) if rc else s, k).reshape(-1, 2)
        for max_dist, max_drift, max_gap, min_len, min_hits in (
                (5000, 500, k, 1, 1), (0, 0, k, 1, 1), (200, 20, 0, 2, 30), (2**31 - 1, 0, k, 1, 1)):
            blocks = blocks_ref.blocks(rows, max_gap, min_len, 1)
            chains, member = chains_ref.chains(blocks, max_dist, max_drift, min_hits)
            for row_free in (0, 1):
                r = R.L.sequence_kmer_chains(ptr, R.s(s), R.i(k), R.i(max_dist), R.i(max_drift),
                                             R.i(max_gap), R.i(min_len), R.i(min_hits), R.i(rc),
                                             R.i(row_free))
                what = (rc, max_dist, max_drift, max_gap, min_len, min_hits, row_free)
                assert R.L.fr_type(r) == VECSXP and R.L.fr_len(r) == 3
                assert R.strings(R.L.fr_names(r)) == ["chains", "blocks", "chain"]
                c, b, m = (R.L.fr_elt(r, j) for j in range(3))
                assert [R.L.fr_type(x) for x in (c, b, m)] == [INTSXP] * 3
                assert (R.L.fr_nrow(c), R.L.fr_ncol(c)) == (6, len(chains)), what
                assert (R.L.fr_nrow(b), R.L.fr_ncol(b)) == (4, len(blocks)), what
                assert R.L.fr_len(m) == len(blocks) > 0
                assert np.array_equal(R.int_matrix(c), chains), what      # (C, 6): R's t(m)
                assert np.array_equal(R.int_matrix(b), blocks), what
                got = np.ctypeslib.as_array(R.L.fr_ints(m), shape=(len(blocks),))
                assert np.array_equal(got, member), what
    assert R.L.fr_finalize(ptr) == 1
