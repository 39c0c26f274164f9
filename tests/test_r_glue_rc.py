"""The R glue's sequence_kmer_positions_rc (seq.kmer.pos.rc) over tests/rshim (see
tests/test_r_glue.py for the stand-in R runtime).  Like count_kmers_fastq_sh it is exported from
the glue but not in its registration table, which stays pinned to the reference's names, so it
is called here by symbol, as R's .Call by name finds it through its dynamic lookup."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
from test_r_glue import INTSXP, ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    f = r.L.sequence_kmer_positions_rc
    f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * 3
    yield r
    r.L.fr_reset()


def test_entry_point_exported_wrapped_and_not_registered(R):
    assert R.L.sequence_kmer_positions_rc
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    # seq.kmer.pos's own shape: row names i, j and transposed
    assert ('seq.kmer.pos.rc <- function(ex.ptr, seq, k){ m <- .Call("sequence_kmer_positions_rc", '
            'ex.ptr, as.character(seq), as.integer(k)) rownames(m) <- c("i", "j") t(m) }') in txt
    assert "nchar(seq) - i + 1" in txt                    # the coordinate formula is documented
    got = {}
    for j in range(R.n_routines):
        n = C.c_int()
        name = R.L.fr_routine(j, C.byref(n)).decode()
        got[name] = n.value
    # the registration table is still the reference's (src/kmer_hash.c:1205-1219) + kmer_row_order
    ref = {"make_kmer_h_index": 3, "kmer_positions": 2, "sequence_kmer_positions": 3,
           "kmer_pair_pos": 2, "count_kmers": 3, "count_kmers_fastq_sh_rp": 3,
           "seq_kmer_depth_sh": 3, "kmer_spectrum_suffix_hash_n": 5}
    for name, n in ref.items():
        assert got.get(name) == n, name
    assert set(got) - set(ref) == {"kmer_row_order"}


@pytest.mark.gpu
def test_testfa_matrix_equals_the_oracle(gpu, R, testfa):
    k = 15
    ptr = R.call("make_kmer_h_index", R.s(testfa), R.i(k), R.i(0))
    m = R.L.sequence_kmer_positions_rc(ptr, R.s(testfa), R.i(k))
    assert R.L.fr_type(m) == INTSXP and R.L.fr_nrow(m) == 2
    got = R.int_matrix(m)
    want = O.OracleIndex(testfa, k).query(rc_host(testfa), k)
    assert got.shape == (len(want) // 2, 2) and len(want) > 0
    assert np.array_equal(got.reshape(-1), want)
    # the forward entry through the same shared body is unchanged
    f = R.int_matrix(R.call("sequence_kmer_positions", ptr, R.s(testfa), R.i(k)))
    assert np.array_equal(f.reshape(-1), O.OracleIndex(testfa, k).query(testfa, k))
    assert R.L.fr_finalize(ptr) == 1
