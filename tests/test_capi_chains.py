"""The chains entries of the C-ABI (kmhg_blocks_chains, kmhg_chains_run*, kmhg_chains_*): null,
out-of-range and zero-size arguments are answered before any device work (CPU-safe) in the
header's order, an empty result is a real handle, and a handle nobody read is freed."""
import ctypes as C

import numpy as np
import pytest

from kmer_hasher_amd import _lib

MAXDIST = "max_dist must not be negative"
MAXDRIFT = "max_drift must not be negative"
MINHITS = "min_hits must be a positive integer"
MINLEN = "min_len must be a positive integer"
MAXGAP = "max_gap must not be negative"
COUNT = "bad block count"


def _err(L):
    return L.kmhg_last_error().decode()


def test_null_and_bad_arguments_are_einval_in_order():
    L = _lib.lib()
    g, n = C.c_void_p(), C.c_int64(-7)
    dummy = C.c_void_p(16)                           # never read: refused first
    out = (C.byref(g), C.byref(n))
    # every argument wrong at once: the first check in the header's order answers
    assert L.kmhg_blocks_chains(dummy, -1, -1, -1, 0, None, None, C.byref(n)) == _lib.KMHG_EINVAL
    assert _err(L) == "null argument"
    assert L.kmhg_blocks_chains(dummy, -1, -1, -1, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MAXDIST
    assert L.kmhg_blocks_chains(dummy, -1, 0, -1, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MAXDRIFT
    assert L.kmhg_blocks_chains(dummy, -1, 0, 0, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MINHITS
    assert L.kmhg_blocks_chains(dummy, -1, 0, 0, 1, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == COUNT
    for bad in (-1, -2**40):
        for d_blocks, blocks in ((dummy, 5), (None, 0)):
            assert L.kmhg_blocks_chains(d_blocks, blocks, bad, 3, 1, None, *out) == _lib.KMHG_EINVAL
            assert _err(L) == MAXDIST
            assert L.kmhg_blocks_chains(d_blocks, blocks, 3, bad, 1, None, *out) == _lib.KMHG_EINVAL
            assert _err(L) == MAXDRIFT
            assert L.kmhg_blocks_chains(d_blocks, blocks, 3, 3, bad, None, *out) == _lib.KMHG_EINVAL
            assert _err(L) == MINHITS
    assert L.kmhg_blocks_chains(dummy, 5, 3, 3, 0, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == MINHITS
    for bad in (-1, 2**31, 2**40):
        assert L.kmhg_blocks_chains(dummy, bad, 0, 0, 1, None, *out) == _lib.KMHG_EINVAL
        assert _err(L) == COUNT
    assert L.kmhg_blocks_chains(None, 5, 0, 0, 1, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == "null argument"
    assert L.kmhg_blocks_chains(C.c_void_p(24), 5, 0, 0, 1, None, *out) == _lib.KMHG_EINVAL
    assert _err(L) == "blocks must be 16-byte aligned"
    d = C.c_void_p()
    assert L.kmhg_chains_device(None, C.byref(d), C.byref(n), None, None, None) == _lib.KMHG_EINVAL
    assert L.kmhg_chains_copy_device(None, dummy, dummy, None, None) == _lib.KMHG_EINVAL
    assert L.kmhg_chains_fill(None, None) == _lib.KMHG_EINVAL
    assert L.kmhg_chains_member_fill(None, None, None) == _lib.KMHG_EINVAL
    assert not g.value and n.value == -7             # nothing was written on a refusal
    assert L.kmhg_chains_free(None) == _lib.KMHG_OK


def test_run_entries_refuse_in_the_blocks_entries_order():
    L = _lib.lib()
    g = C.c_void_p()
    nc, nb, nr = C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    tail = (C.byref(g), C.byref(nc), C.byref(nb), C.byref(nr))
    idx, seq = C.c_void_p(16), C.c_void_p(16)        # never read: refused first
    for row_free in (0, 1):
        def dev(*p, out=tail, i=idx, s=seq):
            return L.kmhg_chains_run_device(i, s, 100, 15, 0, row_free, *p, None, *out)

        def host(*p, out=tail, i=idx, s=b"ACGT"):
            return L.kmhg_chains_run(i, s, 4, 15, 0, row_free, *p, *out)

        for f in (dev, host):
            assert f(0, -1, -1, -1, 0, i=None) == _lib.KMHG_EINVAL and _err(L) == "null argument"
            assert f(0, -1, -1, -1, 0, s=None) == _lib.KMHG_EINVAL and _err(L) == "null argument"
            assert f(0, -1, -1, -1, 0, out=(None,) + tail[1:]) == _lib.KMHG_EINVAL
            assert _err(L) == "null argument"
            # min_len, max_gap, max_dist, max_drift, min_hits
            assert f(0, -1, -1, -1, 0) == _lib.KMHG_EINVAL and _err(L) == MINLEN
            assert f(1, -1, -1, -1, 0) == _lib.KMHG_EINVAL and _err(L) == MAXGAP
            assert f(1, 0, -1, -1, 0) == _lib.KMHG_EINVAL and _err(L) == MAXDIST
            assert f(1, 0, 0, -1, 0) == _lib.KMHG_EINVAL and _err(L) == MAXDRIFT
            assert f(1, 0, 0, 0, 0) == _lib.KMHG_EINVAL and _err(L) == MINHITS
        # then the query entries' own, before the index is read: k out of range
        assert L.kmhg_chains_run_device(idx, seq, 100, 0, 0, row_free, 1, 0, 0, 0, 1, None,
                                        *tail) == _lib.KMHG_EINVAL
        assert L.kmhg_chains_run_device(idx, seq, 100, -1, 0, row_free, 1, 0, 2**40, 2**40, 2**40,
                                        None, *tail) == _lib.KMHG_EINVAL
    assert not g.value and nc.value == nb.value == nr.value == -7


def test_no_blocks_give_an_empty_handle_without_reading_d_blocks():
    L = _lib.lib()
    for d_blocks in (None, C.c_void_p(16)):          # 16 is no device address: it is not read
        for md, mr, mh in ((0, 0, 1), (5000, 500, 7), (2**40, 2**40, 2**40)):   # beyond int32: legal
            g, n = C.c_void_p(), C.c_int64(-1)
            assert L.kmhg_blocks_chains(d_blocks, 0, md, mr, mh, None, C.byref(g), C.byref(n)) == \
                _lib.KMHG_OK
            assert g.value and n.value == 0
            d, m, b = C.c_void_p(123), C.c_void_p(123), C.c_void_p(123)
            nc, nb = C.c_int64(-1), C.c_int64(-1)
            assert L.kmhg_chains_device(g, C.byref(d), C.byref(nc), C.byref(m), C.byref(b),
                                        C.byref(nb)) == _lib.KMHG_OK
            assert not d.value and not m.value and not b.value and nc.value == nb.value == 0
            assert L.kmhg_chains_device(g, C.byref(d), None, None, None, None) == _lib.KMHG_OK
            assert L.kmhg_chains_device(g, None, None, None, None, None) == _lib.KMHG_EINVAL
            assert L.kmhg_chains_fill(g, None) == _lib.KMHG_OK          # nothing to write
            assert L.kmhg_chains_member_fill(g, None, None) == _lib.KMHG_OK
            assert L.kmhg_chains_copy_device(g, None, None, None, None) == _lib.KMHG_OK
            # the blocks were the caller's: the handle holds none
            host = np.empty(4, np.int32)
            assert L.kmhg_chains_member_fill(g, None, host.ctypes.data) == _lib.KMHG_EINVAL
            assert _err(L) == "the handle holds no blocks"
            assert L.kmhg_chains_copy_device(g, None, None, C.c_void_p(16), None) == \
                _lib.KMHG_EINVAL
            assert L.kmhg_chains_free(g) == _lib.KMHG_OK
    g = C.c_void_p()
    assert L.kmhg_blocks_chains(None, 0, 0, 0, 1, None, C.byref(g), None) == _lib.KMHG_OK
    assert L.kmhg_chains_free(g) == _lib.KMHG_OK     # a handle nobody read (n_chains optional)


@pytest.mark.gpu
def test_unused_and_partly_used_handles_are_freed(gpu):
    torch = gpu
    L = _lib.lib()
    blocks = torch.tensor([(1, 1, 4, 4), (2, 50, 1, 1), (6, 6, 2, 2), (90, 90, 3, 3)],
                          dtype=torch.int32, device="cuda")
    p = C.c_void_p(blocks.data_ptr())
    g, n = C.c_void_p(), C.c_int64()
    _lib.check(L.kmhg_blocks_chains(p, 4, 9, 9, 1, None, C.byref(g), C.byref(n)))
    assert n.value == 3
    _lib.check(L.kmhg_chains_free(g))                # never read
    _lib.check(L.kmhg_blocks_chains(p, 4, 9, 9, 2, None, C.byref(g), None))
    assert L.kmhg_chains_fill(g, None) == _lib.KMHG_EINVAL and _err(L) == "null output"
    assert L.kmhg_chains_member_fill(g, None, None) == _lib.KMHG_EINVAL and _err(L) == "null output"
    assert L.kmhg_chains_copy_device(g, None, None, None, None) == _lib.KMHG_EINVAL
    assert _err(L) == "null output"
    host, member = np.empty(12, np.int32), np.empty(4, np.int32)
    _lib.check(L.kmhg_chains_fill(g, host.ctypes.data))
    _lib.check(L.kmhg_chains_member_fill(g, member.ctypes.data, None))
    assert host.tolist() == [1, 1, 7, 7, 6, 2, 90, 90, 92, 92, 3, 1]
    assert member.tolist() == [1, 0, 1, 2]
    dc = torch.zeros(12, dtype=torch.int32, device="cuda")
    dm = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    _lib.check(L.kmhg_chains_copy_device(g, C.c_void_p(dc.data_ptr()), C.c_void_p(dm.data_ptr()),
                                         None, None))
    torch.cuda.synchronize()
    assert dc.cpu().tolist() == host.tolist() and dm.cpu().tolist() == [1, 0, 1, 2]
    d, m, b = C.c_void_p(), C.c_void_p(), C.c_void_p(5)
    nc, nb = C.c_int64(), C.c_int64()
    _lib.check(L.kmhg_chains_device(g, C.byref(d), C.byref(nc), C.byref(m), C.byref(b),
                                    C.byref(nb)))
    assert d.value and m.value and not b.value and (nc.value, nb.value) == (2, 4)
    _lib.check(L.kmhg_chains_free(g))
    _lib.check(L.kmhg_blocks_chains(p, 4, 9, 9, 2**40, None, C.byref(g), C.byref(n)))   # all dropped
    assert n.value == 0
    _lib.check(L.kmhg_chains_member_fill(g, member.ctypes.data, None))
    assert member.tolist() == [0, 0, 0, 0]
    _lib.check(L.kmhg_chains_free(g))


@pytest.mark.gpu
@pytest.mark.parametrize("blocks,message", [
    ([(1, 2, 1, 1), (1, 2, 1, 1)], "blocks are not in ascending (i, j) order"),
    ([(2, 1, 1, 1), (1, 9, 1, 1)], "blocks are not in ascending (i, j) order"),
    ([(1, 1, 0, 1)], "blocks must have i, j >= 1, 1 <= hits <= span and ends within 2^31 - 1"),
    ([(1, 1, 2, 3)], "blocks must have i, j >= 1, 1 <= hits <= span and ends within 2^31 - 1"),
    ([(1, 1, 2, 0)], "blocks must have i, j >= 1, 1 <= hits <= span and ends within 2^31 - 1"),
    ([(2, 1, 2**31 - 1, 1)],
     "blocks must have i, j >= 1, 1 <= hits <= span and ends within 2^31 - 1"),
])
def test_faulty_blocks_are_refused_from_the_device(gpu, blocks, message):
    torch = gpu
    L = _lib.lib()
    t = torch.tensor(blocks, dtype=torch.int32, device="cuda")
    g, n = C.c_void_p(), C.c_int64(-7)
    assert L.kmhg_blocks_chains(C.c_void_p(t.data_ptr()), len(blocks), 9, 9, 1, None, C.byref(g),
                                C.byref(n)) == _lib.KMHG_EINVAL
    assert _err(L) == message
    assert not g.value and n.value == -7
