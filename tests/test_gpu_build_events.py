"""The build's one event and the pool's unfenced release events, against the oracle.

A partitioned build records a single event on its stream: the pinned totals record's, which the
scratch buffers' release group adopts; an index freed before its first use releases its own
buffers behind the same event.  The pool's own release events carry no system-scope fence.  These
tests push blocks through those paths as fast as the host can enqueue -- builds freed unwaited,
reuse across streams, totals read right after the build -- and compare every result with the
oracle, so a block handed out early or a stale pinned record shows as wrong totals or rows.
No case retries: the first difference fails the test."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

K = 31


def _totals(inf):
    return inf["n_kmers"], inf["n_positions"], inf["n_pairs"], inf["max_count"]


def _oracle_totals(oi):
    return oi.U, oi.N, oi.P, int(oi.counts.max())


def _seq(torch, n, seed):
    """iid bases with three copied stretches (repeated k-mers, pairs) and two runs of N."""
    from kmer_hasher_amd import synth
    s = synth.iid(n, seed).copy()
    w = n // 20
    for src, dst in ((0, 7 * w), (2 * w, 11 * w), (2 * w, 15 * w)):
        s[dst:dst + w] = s[src:src + w]
    s[5 * w:5 * w + 40] = ord("N")
    s[13 * w + 3:13 * w + 4] = ord("N")
    return s, torch.from_numpy(s).cuda()


# 5,000 bases: three partition tiles, one bucket-kernel round; 300,000: two radix passes
@pytest.mark.parametrize("n,builds", [(5_000, 40), (300_000, 10)])
def test_back_to_back_builds_freed_without_a_wait(gpu, n, builds):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    s, t = _seq(torch, n, 21)
    oi = O.OracleIndex(s.tobytes(), K)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(builds - 1):
            DeviceIndex.build(t, K, stream).free()
        idx = DeviceIndex.build(t, K, stream)
        inf = idx.info()
        assert inf["fallback"] == 0
        assert _totals(inf) == _oracle_totals(oi)
        q = idx.query(t, K, stream)
        assert np.array_equal(q.rows().cpu().numpy().reshape(-1), oi.query(s.tobytes(), K))
        q.free()
        idx.free()
    stream.synchronize()


def test_blocks_freed_on_one_stream_are_reused_by_a_build_on_another(gpu):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    n = 300_000
    sa, ta = _seq(torch, n, 31)
    sb, tb = _seq(torch, n, 32)
    ob = O.OracleIndex(sb.tobytes(), K)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()                      # both inputs are in place for either stream
    DeviceIndex.build(ta, K, A).free()            # in flight on A; its blocks wait for its event
    idx = DeviceIndex.build(tb, K, B)             # same sizes: the same blocks, now on B
    inf = idx.info()
    assert inf["fallback"] == 0
    assert _totals(inf) == _oracle_totals(ob)
    q = idx.query(tb, K, B)
    assert np.array_equal(q.rows().cpu().numpy().reshape(-1), ob.query(sb.tobytes(), K))
    q.free()
    idx.free()
    torch.cuda.synchronize()


def test_totals_read_right_after_each_build_are_that_builds(gpu):
    """Two 2,100-base strings with different totals, built in turn 200 times; info() follows each
    build at once.  A pinned record read before the build's write had reached the host would
    show zeros or the other string's totals."""
    torch = gpu
    from kmer_hasher_amd import synth
    from kmer_hasher_amd.device import DeviceIndex
    n = 2_100
    x = synth.iid(n, 41)
    y = synth.iid(n, 42).copy()
    y[700:900] = ord("N")                         # fewer windows, so fewer k-mers
    y[1500:1700] = y[1000:1200]                   # and a repeat: pairs, max_count 2
    seqs = [x, y]
    dev = [torch.from_numpy(v).cuda() for v in seqs]
    want = [_oracle_totals(O.OracleIndex(v.tobytes(), K)) for v in seqs]
    assert want[0] != want[1] and want[0][0] != want[1][0]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for i in range(200):
        idx = DeviceIndex.build(dev[i & 1], K, stream)
        got = _totals(idx.info())
        idx.free()
        assert got == want[i & 1], (i, got, want[i & 1], want[1 - (i & 1)])
    stream.synchronize()
