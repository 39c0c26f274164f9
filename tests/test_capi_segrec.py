"""The row-free segment and block entries of the C-ABI (kmhg_segments_run_device,
kmhg_segments_run, kmhg_blocks_run_device, kmhg_blocks_run): null arguments, the parameters and
the query's k / L are answered before any device work (CPU-safe), in the header's order and
words."""
import ctypes as C

from kmer_hasher_amd import _lib

NULL = "null argument"
MIN_LEN = "min_len must be a positive integer"
MAX_GAP = "max_gap must not be negative"
MIN_HITS = "min_hits must be a positive integer"
QUERY = "the sequence should be longer than k and k should not be longer than 31"
LONG = "sequence longer than 2^31-1 (int positions)"


def _err(L):
    return L.kmhg_last_error().decode()


def _entries(L, dummy, n, k, min_len=1, max_gap=0, min_hits=1, idx=True, seq=True, out=True):
    """The four entries called with the same faults: (is a blocks entry, return code, word)."""
    g, a, b = C.c_void_p(), C.c_int64(-7), C.c_int64(-7)
    i = dummy if idx else None
    o = C.byref(g) if out else None
    d = dummy if seq else None
    h = b"ACGTACGTACGT" if seq else None
    got = []
    for blocks, call in (
            (False, lambda: L.kmhg_segments_run_device(i, d, n, k, 0, min_len, None, o, C.byref(a),
                                                       C.byref(b))),
            (False, lambda: L.kmhg_segments_run(i, h, n, k, 1, min_len, o, C.byref(a), C.byref(b))),
            (True, lambda: L.kmhg_blocks_run_device(i, d, n, k, 0, min_len, max_gap, min_hits, None,
                                                    o, C.byref(a), C.byref(b))),
            (True, lambda: L.kmhg_blocks_run(i, h, n, k, 1, min_len, max_gap, min_hits, o,
                                             C.byref(a), C.byref(b)))):
        rc = call()
        got.append((blocks, rc, _err(L)))
    assert g.value is None and a.value == -7 and b.value == -7      # nothing written on a refusal
    return got


def test_refusals_before_any_device_work_in_the_headers_order():
    L = _lib.lib()
    dummy = C.c_void_p(16)                           # never read: refused first
    # every later fault is present too: the earlier word wins
    for kw in (dict(idx=False), dict(seq=False), dict(out=False)):
        for _, rc, word in _entries(L, dummy, 3, 40, 0, -1, 0, **kw):
            assert rc == _lib.KMHG_EINVAL and word == NULL
    for blocks, rc, word in _entries(L, dummy, 3, 40, 0, -1, 0):
        assert rc == _lib.KMHG_EINVAL and word == MIN_LEN
    for blocks, rc, word in _entries(L, dummy, 3, 40, -5, 0, 1):
        assert rc == _lib.KMHG_EINVAL and word == MIN_LEN
    for blocks, rc, word in _entries(L, dummy, 3, 40, 1, -1, 0):
        assert rc == _lib.KMHG_EINVAL and word == (MAX_GAP if blocks else QUERY)
    for blocks, rc, word in _entries(L, dummy, 3, 40, 2**40, 2**40, 0):
        assert rc == _lib.KMHG_EINVAL and word == (MIN_HITS if blocks else QUERY)
    # k and L as the query entries refuse them, after legal parameters (beyond int32 is legal)
    for n, k in ((3, 3), (12, 12), (12, 32), (12, 0), (12, -1), (0, 5)):
        for _, rc, word in _entries(L, dummy, n, k, 2**40, 2**40, 2**40):
            assert rc == _lib.KMHG_EINVAL and word == QUERY
    # the device entries refuse a length beyond int positions (the host entries read the string,
    # which ends at its NUL)
    g, a = C.c_void_p(), C.c_int64()
    assert L.kmhg_segments_run_device(dummy, dummy, 2**31 - 1, 15, 0, 1, None, C.byref(g), None,
                                      C.byref(a)) == _lib.KMHG_EOVERFLOW and _err(L) == LONG
    assert L.kmhg_blocks_run_device(dummy, dummy, 2**40, 15, 1, 1, 0, 1, None, C.byref(g), None,
                                    C.byref(a)) == _lib.KMHG_EOVERFLOW and _err(L) == LONG
    assert g.value is None


def test_prototypes_are_declared():
    for name in ("kmhg_segments_run_device", "kmhg_segments_run", "kmhg_blocks_run_device",
                 "kmhg_blocks_run"):
        assert getattr(_lib.lib(), name).restype is C.c_int
