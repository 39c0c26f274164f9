"""reads.kmer.pos / reads.kmer.vote at the C entries, without a device: the entries exist with the
declared prototypes, and the refusals that are decided before any device call return their code
and message."""
import ctypes as C

import numpy as np
import pytest

from kmer_hasher_amd import _lib, api

ENTRIES = ["kmhg_reads_query_run_device", "kmhg_reads_query_run_packed", "kmhg_reads_query_run",
           "kmhg_rquery_rows_device", "kmhg_rquery_copy_device", "kmhg_rquery_fill",
           "kmhg_rquery_free", "kmhg_rrows_votes", "kmhg_rquery_votes", "kmhg_rquery_votes_device"]


def _err():
    return _lib.lib().kmhg_last_error().decode()


def test_entries_are_declared_and_exported():
    L = _lib.lib()
    syms = _lib.header_symbols()
    for name in ENTRIES:
        assert name in syms and name in _lib._PROTOS
        assert getattr(L, name).argtypes == _lib._PROTOS[name][1]


def test_null_arguments_are_refused():
    L = _lib.lib()
    q, h = C.c_void_p(), C.c_int64()
    off = np.zeros(1, np.int64)
    assert L.kmhg_reads_query_run_packed(None, None, 0, off.ctypes.data, 0, 15, 3, C.byref(q),
                                         C.byref(h)) == _lib.KMHG_EINVAL
    assert _err() == "null argument"
    assert L.kmhg_reads_query_run_device(None, None, 0, None, 0, 15, 3, None, C.byref(q),
                                         C.byref(h)) == _lib.KMHG_EINVAL
    assert L.kmhg_reads_query_run(None, None, 15, 3, C.byref(q), C.byref(h)) == _lib.KMHG_EINVAL
    assert L.kmhg_rquery_fill(None, None) == _lib.KMHG_EINVAL and _err() == "null query"
    assert L.kmhg_rquery_votes(None, 64, None) == _lib.KMHG_EINVAL
    assert L.kmhg_rquery_free(None) == _lib.KMHG_OK


@pytest.mark.parametrize("args,code,text", [
    ((10, 3, 15, 0), _lib.KMHG_EINVAL, "band must be between 1 and 2^30"),
    ((10, 3, 15, 2**30 + 1), _lib.KMHG_EINVAL, "band must be between 1 and 2^30"),
    ((10, 3, 0, 64), _lib.KMHG_EINVAL, "k should be between 1 and 31"),
    ((10, 3, 32, 64), _lib.KMHG_EINVAL, "k should be between 1 and 31"),
    ((-1, 3, 15, 64), _lib.KMHG_EINVAL, "negative row or read count"),
    ((2**31, 3, 15, 64), _lib.KMHG_EOVERFLOW, "more than 2^31-1 rows in one vote: split the rows"),
    ((10, 2**31, 15, 64), _lib.KMHG_EOVERFLOW, "more than 2^31-1 reads in one call: split the reads"),
])
def test_vote_refusals_launch_nothing(args, code, text):
    """Null device pointers: a refusal that came after a launch would have used them."""
    n_rows, n_reads, k, band = args
    assert _lib.lib().kmhg_rrows_votes(None, n_rows, n_reads, k, band, None, None) == code
    assert _err() == text


def test_host_api_refuses_before_the_library():
    ptr = api.ExtPtr(0)
    for bad_k in (0, 32, [15, 16]):
        with pytest.raises(api.KmerHashError):
            api.reads_kmer_pos(ptr, ["ACGT"], bad_k)
    with pytest.raises(api.KmerHashError):
        api.reads_kmer_pos(ptr, ["ACGT"], 3, strand="sideways")
    with pytest.raises(api.KmerHashError):
        api.reads_kmer_vote(ptr, ["ACGT"], 3, band=0)
    with pytest.raises(api.KmerHashError):
        api.reads_kmer_pos("not a pointer", ["ACGT"], 3)
