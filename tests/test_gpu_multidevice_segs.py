"""seq.kmer.segs of a multi-device query (KMHG_DEVICES, tests/test_gpu_multidevice.py): the
handle holds one part per device, kmhg_query_segments gathers them on the index's device, as the
device-side readers do, and the segments equal the single-device query's -- segments that cross
a part boundary included."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import segs_ref
from test_gpu_multidevice import _devices_list

pytestmark = pytest.mark.gpu


def test_two_part_query_gives_the_single_device_segments(gpu, test_lib, monkeypatch):
    from kmer_hasher_amd import _lib, api, synth
    A = synth.add_n_runs(synth.iid(60_000, 171), 0.0005, 172, max_run=40)
    B = synth.derived(A, 173).tobytes()
    s = A.tobytes()
    k = 21
    want = segs_ref.segments(O.OracleIndex(s, k).query(B, k).reshape(-1, 2))
    assert len(want) > 10 and want[:, 2].max() > 100
    ptr = api.make_kmer_hash(s, k)
    single = api.seq_kmer_segs(ptr, B, k)
    assert np.array_equal(single, want)
    monkeypatch.setenv("KMHG_DEVICES", _devices_list(gpu, 2))
    monkeypatch.setenv("KMHG_TEST_REPLICA", "1")
    L = _lib.lib()
    q, h = C.c_void_p(), C.c_int64()
    _lib.check(L.kmhg_query_run(ptr.handle, B, len(B), k, C.byref(q), C.byref(h)))
    assert h.value == want[:, 2].sum()
    for ml in (1, 50):
        g, n = C.c_void_p(), C.c_int64()
        _lib.check(L.kmhg_query_segments(q, ml, C.byref(g), C.byref(n)))
        got = np.empty(3 * n.value, np.int32)
        _lib.check(L.kmhg_segs_fill(g, got.ctypes.data))
        _lib.check(L.kmhg_segs_free(g))
        assert np.array_equal(got.reshape(-1, 3), want[want[:, 2] >= ml]), ml
    _lib.check(L.kmhg_query_free(q))
    assert np.array_equal(api.seq_kmer_segs(ptr, B, k, min_len=2), want[want[:, 2] >= 2])
    ptr.free()
