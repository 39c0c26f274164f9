"""The raster entries of the C-ABI (kmhg_rows_raster, kmhg_query_raster, kmhg_raster_run_device,
kmhg_raster_run): null arguments and illegal frames are answered before any device work
(CPU-safe), in the header's order and words."""
import ctypes as C

import pytest

from kmer_hasher_amd import _lib

M = 2**31 - 1
NULL = "null argument"
WIDTH = "bin widths must be positive integers"
COUNT = "bin counts must be positive integers"
CELLS = "a raster has at most 2^26 cells"
FRAME = "the frame must lie within 1..2^31-1 on both axes"

# every later fault is present too: the earlier word wins
ORDER = [((0, 0, 0, 1, 0, 2**30), WIDTH), ((0, 0, 1, -3, -1, 2**30), WIDTH),
         ((0, 0, 1, 1, 0, 2**30), COUNT), ((0, 0, 1, 1, 2**30, -1), COUNT),
         ((0, 0, 1, 1, 2**13, 2**13 + 1), CELLS), ((0, 0, 2**40, 1, 2**62, 2**62), CELLS),
         ((0, 0, 1, 1, 2**26 + 1, 1), CELLS), ((0, 0, 1, 1, 1, 2**27), CELLS),
         ((0, 1, 1, 1, 4, 4), FRAME), ((1, 0, 1, 1, 4, 4), FRAME), ((-5, 1, 1, 1, 4, 4), FRAME),
         ((M, 1, 1, 1, 2, 1), FRAME), ((1, 2, 1, M, 1, 1), FRAME), ((1, 1, 2**31, 1, 1, 1), FRAME),
         ((1, 1, 1, 2**62, 1, 4), FRAME), ((2**31, 1, 1, 1, 1, 1), FRAME),
         ((1, 1, 2**5 + 1, 1, 2**26, 1), FRAME)]


def _err(L):
    return L.kmhg_last_error().decode()


def _frame(f):
    return (C.c_int64 * 6)(*f)


def test_nulls_then_the_frame_in_the_headers_order():
    L = _lib.lib()
    dummy = C.c_void_p(16)                           # never read: refused first
    bad = _frame((0, 0, 0, 0, 0, 0))
    n = C.c_int64(-7)
    for call in (lambda fr, out: L.kmhg_rows_raster(dummy, -1, fr, out, None),
                 lambda fr, out: L.kmhg_query_raster(dummy, fr, out, None),
                 lambda fr, out: L.kmhg_raster_run_device(dummy, dummy, 3, 40, 0, fr, out, None,
                                                          C.byref(n)),
                 lambda fr, out: L.kmhg_raster_run(dummy, b"ACG", 3, 40, 0, fr, out, C.byref(n))):
        assert call(None, dummy) == _lib.KMHG_EINVAL and _err(L) == NULL
        assert call(bad, None) == _lib.KMHG_EINVAL and _err(L) == NULL
    assert L.kmhg_query_raster(None, bad, dummy, None) == _lib.KMHG_EINVAL and _err(L) == NULL
    assert L.kmhg_raster_run_device(None, dummy, 3, 40, 0, bad, dummy, None, None) == \
        _lib.KMHG_EINVAL and _err(L) == NULL
    assert L.kmhg_raster_run_device(dummy, None, 3, 40, 0, bad, dummy, None, None) == \
        _lib.KMHG_EINVAL and _err(L) == NULL
    assert L.kmhg_raster_run(dummy, None, 3, 40, 0, bad, dummy, None) == _lib.KMHG_EINVAL
    assert _err(L) == NULL
    assert n.value == -7


@pytest.mark.parametrize("frame,word", ORDER)
def test_frame_refusals(frame, word):
    """The same word from every entry; the rows entry's row count and the query entries' k / L
    checks come after the frame."""
    L = _lib.lib()
    dummy = C.c_void_p(16)
    fr = _frame(frame)
    assert L.kmhg_rows_raster(dummy, -1, fr, dummy, None) == _lib.KMHG_EINVAL and _err(L) == word
    assert L.kmhg_rows_raster(None, 0, fr, dummy, None) == _lib.KMHG_EINVAL and _err(L) == word
    assert L.kmhg_raster_run_device(dummy, dummy, 3, 40, 0, fr, dummy, None, None) == \
        _lib.KMHG_EINVAL and _err(L) == word
    assert L.kmhg_raster_run(dummy, b"ACG", 3, 40, 1, fr, dummy, None) == _lib.KMHG_EINVAL
    assert _err(L) == word


def test_row_count_and_query_words_follow_a_legal_frame():
    L = _lib.lib()
    dummy = C.c_void_p(16)
    for f in ((1, 1, 1, 1, 1, 1), (M, M, 1, 1, 1, 1), (1, 1, M, M, 1, 1), (1, 1, 1, 1, 2**13, 2**13),
              (1, 1, 2**5 - 1, 1, 2**26, 1), (M - 3, 5, 2, 7, 2, 9)):
        fr = _frame(f)
        for bad in (-1, 2**31, 2**40):
            assert L.kmhg_rows_raster(dummy, bad, fr, dummy, None) == _lib.KMHG_EINVAL
            assert _err(L) == "bad row count"
        assert L.kmhg_rows_raster(None, 5, fr, dummy, None) == _lib.KMHG_EINVAL and _err(L) == NULL
        for seq, n, k in ((b"ACG", 3, 3), (b"ACGTACGT", 8, 32), (b"ACGTACGT", 8, 0)):
            assert L.kmhg_raster_run_device(dummy, dummy, n, k, 0, fr, dummy, None, None) == \
                _lib.KMHG_EINVAL
            assert _err(L) == \
                "the sequence should be longer than k and k should not be longer than 31"
            assert L.kmhg_raster_run(dummy, seq, n, k, 0, fr, dummy, None) == _lib.KMHG_EINVAL
            assert _err(L) == \
                "the sequence should be longer than k and k should not be longer than 31"


def test_bin_rule_of_the_host_api():
    """width = ceil(length / bins), count = ceil(length / width): never more than asked, the
    whole range covered, the last bin the only short one."""
    from kmer_hasher_amd.api import raster_axis
    assert raster_axis(1, 6000, 1000) == (6, 1000)
    assert raster_axis(1, 47000, 1024) == (46, 1022)
    assert raster_axis(100, 2000, 7) == (272, 7)
    assert raster_axis(5, 5, 1024) == (1, 1)
    for lo, hi, bins in ((1, 10, 3), (7, 7, 1), (1, 1025, 1024), (3, 2**31 - 1, 1024), (1, 999, 1000)):
        w, n = raster_axis(lo, hi, bins)
        assert 1 <= n <= bins and (n - 1) * w < hi - lo + 1 <= n * w
