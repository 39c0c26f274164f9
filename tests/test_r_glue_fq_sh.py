"""The R glue's count_kmers_fastq_sh / kmer_spectrum_suffix_hash over tests/rshim (see
tests/test_r_glue.py for the stand-in R runtime).  The two entry points are exported from the
glue but are not in its registration table (that table is pinned to the reference's names by
test_registration_matches_reference), so they are called here by symbol, as R's .Call by name
finds them through its dynamic lookup; error() outside a registered call aborts the stand-in
runtime, so the refusals are covered through the C-ABI and the Python front end instead
(tests/test_fq_sh_ref.py, tests/test_gpu_fq_sh.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fq_sh_inputs as I
from test_r_glue import REALSXP, EXTPTRSXP, ROOT, FakeR

RFILE = os.path.join(ROOT, "kmer_hasher_amd", "R", "kmer_hash_gpu.R")


@pytest.fixture(scope="module")
def R():
    r = FakeR()
    for name, n in (("count_kmers_fastq_sh", 3), ("kmer_spectrum_suffix_hash", 2)):
        f = getattr(r.L, name)
        f.restype, f.argtypes = C.c_void_p, [C.c_void_p] * n
    yield r
    r.L.fr_reset()


def test_entry_points_exported_and_wrapped(R):
    assert R.L.count_kmers_fastq_sh and R.L.kmer_spectrum_suffix_hash
    txt = re.sub(r"\s+", " ", open(RFILE).read())
    # the reference's wrappers, word for word (kmer_hash.R:56-59 and 89-91)
    assert ('count.kmers.fq.sh <- function(fq.file, params, hash.ptr=NULL){ params <- '
            'as.integer(params) .Call("count_kmers_fastq_sh", hash.ptr, params, fq.file); }') in txt
    assert ('kmer.spec.sh <- function(ptr, max.count){ .Call("kmer_spectrum_suffix_hash", ptr, '
            'as.integer(max.count)) }') in txt


@pytest.mark.gpu
def test_calls_return_tagged_pointer_and_spectrum(gpu, R):
    from kmer_hasher_amd import api
    p = os.path.join(I.GOLDEN, "test_10.fastq")
    prm = [20, 1, 20, 100, 30, -1]
    w0 = R.L.fr_warnings()
    ptr = R.L.count_kmers_fastq_sh(R.nil(), R.i(*prm), R.s(p))
    assert R.L.fr_warnings() == w0
    assert R.L.fr_type(ptr) == EXTPTRSXP and R.L.fr_tag(ptr) == b"suffix_hash_250930"
    assert R.L.fr_has_finalizer(ptr) and R.L.fr_addr(ptr)
    # into the same pointer: returned as it is; report_n < 1 raises the reference's warning
    prm0 = [20, 0, 20, 100, 30, -1]
    assert R.L.count_kmers_fastq_sh(ptr, R.i(*prm0), R.s(p)) == ptr
    assert R.L.fr_warnings() == w0 + 1
    assert R.L.fr_last_warning() == b"negative or 0 report n value specified: set to 1e6"
    sp = R.L.kmer_spectrum_suffix_hash(ptr, R.i(7))
    assert R.L.fr_type(sp) == REALSXP and R.L.fr_len(sp) == 8
    got = np.ctypeslib.as_array(R.L.fr_reals(sp), shape=(8,)).copy()
    want = api.count_kmers_fq_sh(p, prm)
    api.count_kmers_fq_sh(p, prm, want)
    assert np.array_equal(got, api.kmer_spec_sh(want, 7)) and got[0] == 0 and got.sum() > 0
    assert R.L.fr_finalize(ptr) == 1
