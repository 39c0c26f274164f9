"""The R glue's sequence_kmer_segments_rf / sequence_kmer_blocks_rf (seq.kmer.segs and
seq.kmer.blocks with row.free=TRUE) over tests/rshim (see tests/test_r_glue.py for the stand-in R
runtime).  Exported from the glue, not registered, so they are called by symbol; the existing
symbols keep their arities.  error() outside a registered call aborts the stand-in runtime after
printing the message, so each refusal runs in a child process of its own; the argument checks
come before any device work (CPU)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_r_glue import INTSXP, ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")
HERE = os.path.dirname(os.path.abspath(__file__))
ARITY = {"sequence_kmer_segments": 5, "sequence_kmer_segments_rf": 5,
         "sequence_kmer_blocks": 7, "sequence_kmer_blocks_rf": 7}


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    for name, n in ARITY.items():
        f = getattr(r.L, name)
        f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * n
    yield r
    r.L.fr_reset()


def test_entry_points_exported_wrapped_and_not_registered(R):
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    assert ('seq.kmer.segs <- function(ex.ptr, seq, k, min.len=1, rc=FALSE, row.free=FALSE){ '
            'if(length(row.free) != 1 || is.na(row.free)) stop("row.free should be TRUE or FALSE") '
            'if(!row.free) return(.seq.kmer.segs.rows(ex.ptr, seq, k, min.len, rc)) '
            'm <- .Call("sequence_kmer_segments_rf", ex.ptr, as.character(seq), as.integer(k), '
            'as.integer(min.len), as.integer(rc)) rownames(m) <- c("i", "j", "len") t(m) }') in txt
    assert ('seq.kmer.blocks <- function(ex.ptr, seq, k, max.gap=k, min.len=1, min.hits=1, '
            'rc=FALSE, row.free=FALSE){ '
            'if(length(row.free) != 1 || is.na(row.free)) stop("row.free should be TRUE or FALSE") '
            'if(!row.free) return(.seq.kmer.blocks.rows(ex.ptr, seq, k, max.gap, min.len, '
            'min.hits, rc)) m <- .Call("sequence_kmer_blocks_rf", ex.ptr, as.character(seq), '
            'as.integer(k), as.integer(max.gap), as.integer(min.len), as.integer(min.hits), '
            'as.integer(rc)) rownames(m) <- c("i", "j", "span", "hits") t(m) }') in txt
    # the dispatchers are bound after the rows-route functions they keep
    assert txt.index(".seq.kmer.segs.rows <- seq.kmer.segs") > \
        txt.index('.Call("sequence_kmer_segments",')
    assert txt.index(".seq.kmer.blocks.rows <- seq.kmer.blocks") > \
        txt.index('.Call("sequence_kmer_blocks",')
    names = set()
    for j in range(R.n_routines):
        n = C.c_int()
        names.add(R.L.fr_routine(j, C.byref(n)).decode())
    assert not (set(ARITY) & names) and "sequence_kmer_positions" in names


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {here!r}); sys.path.insert(0, {root!r})
from test_r_glue import FakeR
R = FakeR()
blocks = {blocks}
f = R.L.sequence_kmer_blocks_rf if blocks else R.L.sequence_kmer_segments_rf
f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * (7 if blocks else 5)
args = dict(ptr=R.nil(), seq=R.s("ACGTACGT"), k=R.i(3), max_gap=R.i(3), min_len=R.i(1),
            min_hits=R.i(1), rc=R.i(0))
args.update({name}={value})
if blocks:
    f(args["ptr"], args["seq"], args["k"], args["max_gap"], args["min_len"], args["min_hits"],
      args["rc"])
else:
    f(args["ptr"], args["seq"], args["k"], args["min_len"], args["rc"])
print("returned")
"""


@pytest.mark.parametrize("blocks,name,value,message", [
    (0, "seq", 'R.s("ACGT", "ACGT")', "seq_r should be a single sequence"),
    (0, "k", "R.d(3.0)", "k should be an integer of length 1"),
    (0, "min_len", "R.i(0)", "min_len must be a positive integer"),
    (0, "rc", "R.nil()", "rc should be an integer of length 1"),
    (0, "ptr", "R.nil()", "ptr_r should be an external pointer"),   # after the argument checks
    (0, "ptr", 'R.L.fr_extptr(None, b"other_tag")', "External pointer has incorrect tag"),
    (1, "seq", "R.i(1)", "seq_r should be a single sequence"),
    (1, "min_len", "R.i(1, 2)", "min_len must be a positive integer"),
    (1, "max_gap", "R.i(-1)", "max_gap must not be negative"),
    (1, "min_hits", "R.i(0)", "min_hits must be a positive integer"),
    (1, "rc", "R.nil()", "rc should be an integer of length 1"),
    (1, "ptr", "R.nil()", "ptr_r should be an external pointer"),
])
def test_refusals_carry_the_rows_routes_words(R, blocks, name, value, message):
    r = subprocess.run([sys.executable, "-c",
                        _CHILD.format(here=HERE, root=ROOT, blocks=blocks, name=name, value=value)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "returned" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert f"fake_r: error() outside a call: {message}\n" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_row_free_equals_the_rows_route_on_both_strands(gpu, R, testfa):
    k = 15
    s = testfa[:6000]
    ptr = R.call("make_kmer_h_index", R.s(s), R.i(k), R.i(0))
    for rc in (0, 1):
        for min_len in (1, 16):
            a = R.L.sequence_kmer_segments(ptr, R.s(s), R.i(k), R.i(min_len), R.i(rc))
            b = R.L.sequence_kmer_segments_rf(ptr, R.s(s), R.i(k), R.i(min_len), R.i(rc))
            assert R.L.fr_type(b) == INTSXP and R.L.fr_nrow(b) == 3
            assert R.L.fr_ncol(b) == R.L.fr_ncol(a) and (rc or R.L.fr_ncol(a) > 1000)
            assert np.array_equal(R.int_matrix(a), R.int_matrix(b)), (rc, min_len)
        for max_gap, min_len, min_hits in ((0, 1, 1), (k, 1, 1), (100, 2, 50), (2**31 - 1, 1, 1)):
            a = R.L.sequence_kmer_blocks(ptr, R.s(s), R.i(k), R.i(max_gap), R.i(min_len),
                                         R.i(min_hits), R.i(rc))
            b = R.L.sequence_kmer_blocks_rf(ptr, R.s(s), R.i(k), R.i(max_gap), R.i(min_len),
                                            R.i(min_hits), R.i(rc))
            assert R.L.fr_type(b) == INTSXP and R.L.fr_nrow(b) == 4
            assert R.L.fr_ncol(b) == R.L.fr_ncol(a) and (rc or R.L.fr_ncol(a) > 0)
            assert np.array_equal(R.int_matrix(a), R.int_matrix(b)), (rc, max_gap, min_len)
    assert R.L.fr_finalize(ptr) == 1
