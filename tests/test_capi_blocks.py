"""The blocks entries of the C-ABI (kmhg_rows_blocks, kmhg_query_blocks, kmhg_blocks_*): null,
out-of-range and zero-size arguments are answered before any device work (CPU-safe) in the
header's order, an empty result is a real handle, and a handle nobody read is freed."""
import ctypes as C

import numpy as np
import pytest

from kmer_hasher_amd import _lib

MINLEN = "min_len must be a positive integer"
MAXGAP = "max_gap must not be negative"
MINHITS = "min_hits must be a positive integer"


def _err(L):
    return L.kmhg_last_error().decode()


def test_null_and_bad_arguments_are_einval_in_order():
    L = _lib.lib()
    g, n = C.c_void_p(), C.c_int64(-7)
    dummy = C.c_void_p(16)                           # never read: refused first
    out = (C.byref(g), C.byref(n))
    # every argument wrong at once: the first check in the header's order answers
    assert L.kmhg_rows_blocks(dummy, -1, 0, -1, 0, None, None, C.byref(n)) == _lib.KMHG_EINVAL
    assert _err(L) == "null argument"
    assert L.kmhg_rows_blocks(dummy, -1, 0, -1, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MINLEN
    assert L.kmhg_rows_blocks(dummy, -1, 1, -1, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MAXGAP
    assert L.kmhg_rows_blocks(dummy, -1, 1, 0, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MINHITS
    assert L.kmhg_rows_blocks(dummy, -1, 1, 0, 1, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == "bad row count"
    for bad in (0, -1, -2**40):
        for d_rows, rows in ((dummy, 5), (None, 0)):
            assert L.kmhg_rows_blocks(d_rows, rows, bad, 3, 1, None, *out) == _lib.KMHG_EINVAL
            assert _err(L) == MINLEN
            assert L.kmhg_rows_blocks(d_rows, rows, 1, 3, bad, None, *out) == _lib.KMHG_EINVAL
            assert _err(L) == MINHITS
            if bad:
                assert L.kmhg_rows_blocks(d_rows, rows, 1, bad, 1, None, *out) == _lib.KMHG_EINVAL
                assert _err(L) == MAXGAP
    for bad in (-1, 2**31, 2**40):
        assert L.kmhg_rows_blocks(dummy, bad, 1, 0, 1, None, *out) == _lib.KMHG_EINVAL
        assert _err(L) == "bad row count"
    assert L.kmhg_rows_blocks(None, 5, 1, 0, 1, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == "null argument"
    assert L.kmhg_query_blocks(None, 1, 0, 1, *out) == _lib.KMHG_EINVAL
    assert _err(L) == "null argument"
    d = C.c_void_p()
    assert L.kmhg_blocks_device(None, C.byref(d), C.byref(n)) == _lib.KMHG_EINVAL
    assert L.kmhg_blocks_copy_device(None, dummy, None) == _lib.KMHG_EINVAL
    assert L.kmhg_blocks_fill(None, None) == _lib.KMHG_EINVAL
    assert not g.value and n.value == -7             # nothing was written on a refusal
    assert L.kmhg_blocks_free(None) == _lib.KMHG_OK


def test_no_rows_give_an_empty_handle_without_reading_d_rows():
    L = _lib.lib()
    for d_rows in (None, C.c_void_p(16)):            # 16 is no device address: it is not read
        for ml, mg, mh in ((1, 0, 1), (1000, 31, 7), (2**40, 2**40, 2**40)):   # beyond int32: legal
            g, n = C.c_void_p(), C.c_int64(-1)
            assert L.kmhg_rows_blocks(d_rows, 0, ml, mg, mh, None, C.byref(g), C.byref(n)) == \
                _lib.KMHG_OK
            assert g.value and n.value == 0
            d, m = C.c_void_p(123), C.c_int64(-1)
            assert L.kmhg_blocks_device(g, C.byref(d), C.byref(m)) == _lib.KMHG_OK
            assert not d.value and m.value == 0
            assert L.kmhg_blocks_device(g, None, None) == _lib.KMHG_EINVAL
            assert L.kmhg_blocks_fill(g, None) == _lib.KMHG_OK          # nothing to write
            assert L.kmhg_blocks_copy_device(g, None, None) == _lib.KMHG_OK
            assert L.kmhg_blocks_free(g) == _lib.KMHG_OK
    g = C.c_void_p()
    assert L.kmhg_rows_blocks(None, 0, 1, 0, 1, None, C.byref(g), None) == _lib.KMHG_OK
    assert L.kmhg_blocks_free(g) == _lib.KMHG_OK     # a handle nobody read (n_blocks optional)


@pytest.mark.gpu
def test_unused_and_partly_used_handles_are_freed(gpu):
    torch = gpu
    L = _lib.lib()
    rows = torch.tensor([(1, 1), (2, 2), (4, 4), (5, 9)], dtype=torch.int32, device="cuda")
    p = C.c_void_p(rows.data_ptr())
    g, n = C.c_void_p(), C.c_int64()
    _lib.check(L.kmhg_rows_blocks(p, 4, 1, 1, 1, None, C.byref(g), C.byref(n)))
    assert n.value == 2
    _lib.check(L.kmhg_blocks_free(g))                # never read
    _lib.check(L.kmhg_rows_blocks(p, 4, 1, 1, 1, None, C.byref(g), None))
    assert L.kmhg_blocks_fill(g, None) == _lib.KMHG_EINVAL and _err(L) == "null output"
    assert L.kmhg_blocks_copy_device(g, None, None) == _lib.KMHG_EINVAL and _err(L) == "null output"
    host = np.empty(8, np.int32)
    _lib.check(L.kmhg_blocks_fill(g, host.ctypes.data))
    assert host.tolist() == [1, 1, 4, 3, 5, 9, 1, 1]
    dst = torch.zeros(8, dtype=torch.int32, device="cuda")
    _lib.check(L.kmhg_blocks_copy_device(g, C.c_void_p(dst.data_ptr()), None))
    torch.cuda.synchronize()
    assert dst.cpu().tolist() == [1, 1, 4, 3, 5, 9, 1, 1]
    d, m = C.c_void_p(), C.c_int64()
    _lib.check(L.kmhg_blocks_device(g, C.byref(d), C.byref(m)))
    assert d.value and m.value == 2
    _lib.check(L.kmhg_blocks_free(g))
    for ml, mh in ((3, 1), (1, 4), (2**40, 1), (1, 2**40)):       # all filtered out
        _lib.check(L.kmhg_rows_blocks(p, 4, ml, 1, mh, None, C.byref(g), C.byref(n)))
        assert n.value == 0
        _lib.check(L.kmhg_blocks_free(g))
