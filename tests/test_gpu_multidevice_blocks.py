"""seq.kmer.blocks of a multi-device query (KMHG_DEVICES, tests/test_gpu_multidevice.py): the
handle holds one part per device, kmhg_query_blocks gathers them on the index's device, as
kmhg_query_segments does, and the blocks equal the single-device query's -- blocks that cross a
part boundary included.  With one device the parts are replicas on it (KMHG_TEST_REPLICA), as in
test_gpu_multidevice_segs.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import blocks_ref
from test_gpu_multidevice import _devices_list

pytestmark = pytest.mark.gpu


def test_two_part_query_gives_the_single_device_blocks(gpu, test_lib, monkeypatch):
    from kmer_hasher_amd import _lib, api, synth
    A = synth.add_n_runs(synth.iid(60_000, 171), 0.0005, 172, max_run=40)
    B = synth.derived(A, 173).tobytes()
    s = A.tobytes()
    k = 21
    rows = O.OracleIndex(s, k).query(B, k).reshape(-1, 2)
    params = [(0, 1, 1), (k, 1, 1), (k, 2, 50), (2**40, 1, 1)]
    want = [blocks_ref.blocks(rows, *p) for p in params]
    assert len(want[0]) > 10 and len(want[1]) < len(want[0])
    ptr = api.make_kmer_hash(s, k)
    assert np.array_equal(api.seq_kmer_blocks(ptr, B, k), want[1])
    monkeypatch.setenv("KMHG_DEVICES", _devices_list(gpu, 2))
    monkeypatch.setenv("KMHG_TEST_REPLICA", "1")
    L = _lib.lib()
    q, h = C.c_void_p(), C.c_int64()
    _lib.check(L.kmhg_query_run(ptr.handle, B, len(B), k, C.byref(q), C.byref(h)))
    assert h.value == len(rows)
    for (max_gap, min_len, min_hits), w in zip(params, want):
        g, n = C.c_void_p(), C.c_int64()
        _lib.check(L.kmhg_query_blocks(q, min_len, max_gap, min_hits, C.byref(g), C.byref(n)))
        got = np.empty(4 * n.value, np.int32)
        _lib.check(L.kmhg_blocks_fill(g, got.ctypes.data))
        _lib.check(L.kmhg_blocks_free(g))
        assert np.array_equal(got.reshape(-1, 4), w), (max_gap, min_len, min_hits)
    _lib.check(L.kmhg_query_free(q))
    assert np.array_equal(api.seq_kmer_blocks(ptr, B, k, min_len=2, min_hits=50), want[2])
    ptr.free()
