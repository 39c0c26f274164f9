"""The R glue's make_kmer_h_index_min (make.kmer.hash.min) over tests/rshim (see
tests/test_r_glue.py for the stand-in R runtime).  It is exported from the glue but not in its
registration table, so it is called by symbol.  error() outside a registered call aborts the
stand-in runtime after printing the message, so each refusal runs in a child process of its own;
every refusal of an argument is raised before the library is called, so no such child touches the
GPU (CPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import minimizer_ref
from oracle import oracle as O
from test_r_glue import ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    f = r.L.make_kmer_h_index_min
    f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 4
    yield r
    r.L.fr_reset()


def test_entry_point_exported_wrapped_and_not_registered(R):
    assert R.L.make_kmer_h_index_min
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    assert ('make.kmer.hash.min <- function(seq, k, w, do.sort=FALSE){ '
            '.Call("make_kmer_h_index_min", as.character(seq), as.integer(k), as.integer(w), '
            'as.integer(do.sort)) }') in txt
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert "make_kmer_h_index_min" not in names and "make_kmer_h_index" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
f = R.L.make_kmer_h_index_min
f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 4
args = dict(seq=R.s("ACGT" * 20), k=R.i(5), w=R.i(3), sort=R.i(0))
args.update({name}={value})
f(args["seq"], args["k"], args["w"], args["sort"])
print("returned")
"""

ARG = "w should be an integer of length 1"
RANGE = "w must be between 1 and 256"


@pytest.mark.parametrize("name,value,message", [
    ("w", "R.d(3.0)", ARG),                           # the wrapper's as.integer() was skipped
    ("w", 'R.s("3")', ARG),
    ("w", "R.nil()", ARG),
    ("w", "R.i(1, 2)", ARG),
    ("w", "R.i(-2**31)", ARG),                        # NA_integer_
    ("w", "R.i(0)", RANGE),
    ("w", "R.i(257)", RANGE),
    ("w", "R.i(-1)", RANGE),
    ("seq", "R.i(1)", "seq_r should be a character vector of length at least one"),
    ("k", "R.d(5.0)", "k_r must be an integer vector of length at least one"),
    ("k", "R.i(32)", "a sampled index needs k between 1 and 31"),
    ("k", "R.i(80)", "a sampled index needs k between 1 and 31"),
    ("seq", 'R.s("ACGT")', "the length of the sequence must be at least k"),
])
def test_refusals_carry_their_words(R, name, value, message):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD.format(here=HERE, root=ROOT, name=name, value=value)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert f"fake_r: error() outside a call: {message}\n" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_builds_a_sampled_index_and_queries_it(gpu, R, testfa):
    s, k, w = testfa[:6000], 15, 5
    ptr = R.L.make_kmer_h_index_min(R.s(s), R.i(k), R.i(w), R.i(0))
    got = R.int_matrix(R.call("sequence_kmer_positions", ptr, R.s(s), R.i(k)))
    m = minimizer_ref.mask(s, k, w)
    want = minimizer_ref.filter_rows(O.OracleIndex(s, k).query(s, k), k, m, m)
    assert 0 < len(want) and np.array_equal(got, want)
    assert R.L.fr_finalize(ptr) == 1
