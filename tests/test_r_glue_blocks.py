"""The R glue's sequence_kmer_blocks (seq.kmer.blocks) over tests/rshim (see tests/test_r_glue.py
for the stand-in R runtime).  Like sequence_kmer_segments it is exported from the glue but not in
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
from test_r_glue import INTSXP, ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    f = r.L.sequence_kmer_blocks
    f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 7
    yield r
    r.L.fr_reset()


def test_entry_point_exported_wrapped_and_not_registered(R):
    assert R.L.sequence_kmer_blocks
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    assert ('seq.kmer.blocks <- function(ex.ptr, seq, k, max.gap=k, min.len=1, min.hits=1, '
            'rc=FALSE){ m <- .Call("sequence_kmer_blocks", ex.ptr, as.character(seq), '
            'as.integer(k), as.integer(max.gap), as.integer(min.len), as.integer(min.hits), '
            'as.integer(rc)) rownames(m) <- c("i", "j", "span", "hits") t(m) }') in txt
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert "sequence_kmer_blocks" not in names and "sequence_kmer_positions" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
f = R.L.sequence_kmer_blocks
f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 7
args = dict(ptr=R.nil(), seq=R.s("ACGTACGT"), k=R.i(3), max_gap=R.i(3), min_len=R.i(1),
            min_hits=R.i(1), rc=R.i(0))
args.update({name}={value})
f(args["ptr"], args["seq"], args["k"], args["max_gap"], args["min_len"], args["min_hits"],
  args["rc"])
print("returned")
"""


@pytest.mark.parametrize("name,value,message", [
    ("seq", 'R.s("ACGT", "ACGT")', "seq_r should be a single sequence"),
    ("seq", "R.i(1)", "seq_r should be a single sequence"),
    ("k", "R.d(3.0)", "k should be an integer of length 1"),
    ("min_len", "R.i(0)", "min_len must be a positive integer"),
    ("min_len", "R.i(1, 2)", "min_len must be a positive integer"),
    ("max_gap", "R.i(-1)", "max_gap must not be negative"),
    ("max_gap", "R.d(3.0)", "max_gap must not be negative"),
    ("min_hits", "R.i(0)", "min_hits must be a positive integer"),
    ("min_hits", "R.i(-5)", "min_hits must be a positive integer"),
    ("rc", "R.nil()", "rc should be an integer of length 1"),
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
def test_shape_values_strands_and_parameters(gpu, R, testfa):
    k = 15
    s = testfa[:3000]
    a = s[:1500] + rc_host(s[1500:2200]) + s[2200:]          # one inverted stretch
    ptr = R.call("make_kmer_h_index", R.s(a), R.i(k), R.i(0))
    oi = O.OracleIndex(a, k)
    for rc in (0, 1):
        rows = oi.query(rc_host(s) if rc else s, k).reshape(-1, 2)
        for max_gap, min_len, min_hits in ((0, 1, 1), (k, 1, 1), (k, 2, 1), (k, 1, 20),
                                           (2**31 - 1, 1, 1)):
            want = blocks_ref.blocks(rows, max_gap, min_len, min_hits)
            m = R.L.sequence_kmer_blocks(ptr, R.s(s), R.i(k), R.i(max_gap), R.i(min_len),
                                         R.i(min_hits), R.i(rc))
            assert R.L.fr_type(m) == INTSXP and R.L.fr_nrow(m) == 4
            assert R.L.fr_ncol(m) == len(want) > 0
            got = R.int_matrix(m)                            # (B, 4): R's t(m)
            assert got.shape == want.shape and np.array_equal(got, want), (rc, max_gap, min_len)
    assert R.L.fr_finalize(ptr) == 1
