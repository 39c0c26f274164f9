"""seq.kmer.segs -- a seq.kmer.pos result as maximal diagonal segments (kmhg_rows_segments /
kmhg_query_segments, kmhg_segs.hip) -- against tests/segs_ref.py, the numpy restatement of the
definition in include/kmhgpu.h, computed from crafted rows or from the clean-room oracle's rows.
Integer work: every comparison is exact, order included."""
import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import segs_ref
from test_gpu_query_rc import EDGE, _spliced

pytestmark = pytest.mark.gpu

UNSORTED = "rows are not in ascending (i, j) order"
MINLEN = "min_len must be a positive integer"
M = 2**31 - 1


def _segs(torch, rows, min_len=1):
    from kmer_hasher_amd import device
    r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 2))
    t = torch.from_numpy(r).cuda()
    got = device.rows_segments(t, min_len)
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 3 and got.is_cuda
    return got.cpu().numpy()


def _check(torch, rows, min_lens=(1,)):
    """The device's segments of `rows` against segs_ref at every min_len; returns the reference
    at min_len = 1."""
    rows = np.asarray(rows, np.int32).reshape(-1, 2)
    all_ = segs_ref.segments(rows)
    for ml in min_lens:
        got = _segs(torch, rows, ml)
        want = all_[all_[:, 2] >= ml]
        assert got.shape == want.shape and np.array_equal(got, want), (len(rows), ml)
        if ml == 1:                                  # the segments partition the rows
            assert np.array_equal(segs_ref.expand(got), rows)
    return all_


# ------------------------------------------------------------------ 1. crafted rows
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 3 * 2048 + 7])
def test_one_diagonal_and_all_singles(gpu, n):
    t = np.arange(n, dtype=np.int64)
    one = np.stack([t + 1, t + 4], axis=1)
    want = _check(gpu, one, (1, 2, max(n, 1), n + 1))
    assert len(want) == min(n, 1) and (n == 0 or tuple(want[0]) == (1, 4, n))
    singles = np.stack([t + 1, 2 * t + 1], axis=1)   # consecutive windows, never one diagonal
    want = _check(gpu, singles, (1, 2))
    assert len(want) == n and (want[:, 2] == 1).all()


@pytest.mark.parametrize("cut", [2047, 2048, 2049])
def test_segment_crossing_a_tile_boundary(gpu, cut):
    """Rows 0 .. cut - 101 are singles; a diagonal of 200 rows starts at row cut - 100 and so
    crosses row `cut`; singles follow up to 2 tiles + 5 rows."""
    rows, i = [], 1
    for _ in range(cut - 100):
        rows.append((i, 3 * i))
        i += 1
    j0 = 3 * i + 7
    for t in range(200):
        rows.append((i + t, j0 + t))
    i += 200
    while len(rows) < 2 * 2048 + 5:
        rows.append((i, 3 * i + 500))
        i += 1
    want = _check(gpu, rows, (1, 2, 200, 201))
    assert want[cut - 100, 2] == 200 and (np.delete(want[:, 2], cut - 100) == 1).all()


def test_two_interleaved_diagonals(gpu):
    """(i, i) and (i, i + 5) for every i: no row's diagonal neighbour is adjacent in row order,
    so every neighbour test fails and every search succeeds."""
    n = 3 * 2048 + 11
    i = np.arange(1, n + 1, dtype=np.int64)
    rows = np.stack([np.repeat(i, 2), np.stack([i, i + 5], axis=1).reshape(-1)], axis=1)
    want = _check(gpu, rows, (1, n, n + 1))
    assert [tuple(x) for x in want] == [(1, 1, n), (1, 6, n)]


def test_dense_block_every_window_hits_every_position(gpu):
    m = 70                                           # 4,900 rows, 139 diagonals of 1 .. 70 rows
    i, j = np.meshgrid(np.arange(1, m + 1), np.arange(1, m + 1), indexing="ij")
    want = _check(gpu, np.stack([i.reshape(-1), j.reshape(-1)], axis=1), (1, 2, 35, 70, 71))
    assert len(want) == 2 * m - 1 and want[:, 2].max() == m


def test_extreme_coordinates(gpu):
    assert [tuple(x) for x in _check(gpu, [(1, M - 1), (2, M)], (1, 2, 3))] == [(1, M - 1, 2)]
    assert [tuple(x) for x in _check(gpu, [(M - 1, 1), (M, 2)], (1, 2, 3))] == [(M - 1, 1, 2)]
    assert [tuple(x) for x in _check(gpu, [(1, 1)])] == [(1, 1, 1)]      # (0, 0) is never a row
    want = _check(gpu, [(1, 1), (1, M - 1), (2, 2), (2, M), (M - 1, 1), (M - 1, M - 1), (M, 2),
                        (M, M)], (1, 2))
    assert [tuple(x) for x in want] == [(1, 1, 2), (1, M - 1, 2), (M - 1, 1, 2), (M - 1, M - 1, 2)]


def test_bad_rows_and_bad_min_len_are_refused(gpu):
    torch = gpu
    from kmer_hasher_amd import _lib, device
    L = _lib.lib()

    def refused(rows, min_len, msg):
        t = torch.tensor(rows, dtype=torch.int32, device="cuda").reshape(-1, 2)
        with pytest.raises(RuntimeError) as e:
            device.rows_segments(t, min_len)
        assert L.kmhg_last_error().decode() == msg and msg in str(e.value)

    good = [(1, 1), (2, 2), (3, 3)]
    refused([(2, 2), (1, 1), (3, 3)], 1, UNSORTED)
    refused([(1, 5), (1, 4)], 1, UNSORTED)
    refused([(1, 1), (2, 2), (2, 2), (3, 3)], 1, UNSORTED)              # a repeated row
    far = [(i, i) for i in range(1, 5000)]
    far[4100], far[4101] = far[4101], far[4100]                         # in the third tile
    refused(far, 1, UNSORTED)
    refused([(0, 1), (1, 2)], 1, "rows must have i, j >= 1")
    refused(good, 0, MINLEN)
    refused(good, -1, MINLEN)
    refused([], 0, MINLEN)                                              # also with no rows
    assert [tuple(x) for x in _segs(torch, good)] == [(1, 1, 3)]        # and the library goes on


# ------------------------------------------------------------------ 2. oracle rows
def _oracle_rows(index_seq, k, query_seq, kq):
    return O.OracleIndex(index_seq, k).query(query_seq, kq).reshape(-1, 2)


@pytest.mark.parametrize("s,k", EDGE)
def test_edge_strings(gpu, s, k):
    from kmer_hasher_amd import api
    for index_seq in (s, rc_host(s), "ACGTTGCAACGTNACGTAAAATTTT"):
        if len(index_seq) <= k or set(index_seq.upper()) <= {"N"}:
            continue
        ptr = api.make_kmer_hash(index_seq, k)
        for rc in (False, True):
            rows = _oracle_rows(index_seq, k, rc_host(s) if rc else s, k)
            want = segs_ref.segments(rows)
            got = api.seq_kmer_segs(ptr, s, k, rc=rc)
            assert got.dtype == np.int32 and got.shape == want.shape, (s, index_seq, rc)
            assert np.array_equal(got, want), (s, index_seq, rc)
            assert np.array_equal(segs_ref.expand(got), rows)
        ptr.free()


_FA = {}


def _fa(testfa):
    """test.fa[:6000], k = 15, self: the oracle's rows and the reference segments, once."""
    if not _FA:
        s = testfa[:6000]
        rows = _oracle_rows(s, 15, s, 15)
        _FA.update(s=s, rows=rows, want=segs_ref.segments(rows))
    return _FA


def test_testfa_self_is_multi_hit_and_exact(gpu, testfa):
    torch = gpu
    from kmer_hasher_amd import api, device
    fa = _fa(testfa)
    rows, want = fa["rows"], fa["want"]
    H, S = len(rows), len(want)
    assert S * 50 < H                                # the input really is multi-hit
    t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    got = device.rows_segments(t).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(segs_ref.expand(got), rows)
    again = device.rows_segments(t).cpu().numpy()    # determinism: identical bytes
    assert got.tobytes() == again.tobytes()
    # the whole route, and the query handle's entry against rows_segments of its rows
    ptr = api.make_kmer_hash(fa["s"], 15)
    assert np.array_equal(api.seq_kmer_segs(ptr, fa["s"], 15), want)
    ptr.free()


def test_testfa_min_len(gpu, testfa):
    torch = gpu
    from kmer_hasher_amd import device
    fa = _fa(testfa)
    t = torch.from_numpy(np.ascontiguousarray(fa["rows"])).cuda()
    max_len = int(fa["want"][:, 2].max())
    for ml in (1, 2, 16, max_len, max_len + 1):
        want = fa["want"][fa["want"][:, 2] >= ml]
        got = device.rows_segments(t, ml).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), ml
    assert len(fa["want"][fa["want"][:, 2] >= max_len]) >= 1
    assert device.rows_segments(t, max_len + 1).shape == (0, 3)
    assert device.rows_segments(t, 2**40).shape == (0, 3)


def test_short_period_repeat(gpu):
    from kmer_hasher_amd import api
    s = "ACGT" * 600
    rows = _oracle_rows(s, 5, s, 5)
    want = segs_ref.segments(rows)
    assert len(want) * 1000 < len(rows)
    ptr = api.make_kmer_hash(s, 5)
    got = api.seq_kmer_segs(ptr, s, 5)
    assert np.array_equal(got, want) and np.array_equal(segs_ref.expand(got), rows)
    ptr.free()


def test_query_k_differs_from_index_k(gpu, testfa):
    """Index k = 8, query k = 6: the reference hashes the 6-mers against 8-mer keys, so hits are
    coincidences and every segment has one row -- decided from the rows, with no window rule."""
    from kmer_hasher_amd import api
    s = testfa[:5000]
    rows = _oracle_rows(s, 8, s, 6)
    want = segs_ref.segments(rows)
    assert len(rows) > 0 and (want[:, 2] == 1).all()
    ptr = api.make_kmer_hash(s, 8)
    got = api.seq_kmer_segs(ptr, s, 6)
    assert np.array_equal(got, want) and np.array_equal(segs_ref.expand(got), rows)
    ptr.free()


def test_iid_self_is_one_segment(gpu):
    torch = gpu
    from kmer_hasher_amd import synth
    from kmer_hasher_amd.device import DeviceIndex
    k = 31
    s = synth.iid(3 * 2048 + 30, 5)
    rows = _oracle_rows(s, k, s, k)
    want = segs_ref.segments(rows)
    assert len(want) == 1 and want[0, 2] == len(rows) == len(s) - k + 1
    t = torch.from_numpy(s).cuda()
    idx = DeviceIndex.build(t, k)
    q = idx.query(t, k)
    got = q.segments().cpu().numpy()
    assert np.array_equal(got, want)
    q.free()
    idx.free()


@pytest.mark.parametrize("rc", [False, True])
def test_inverted_stretches_both_strands(gpu, rc):
    """An iid query against an index with three inverted stretches: forward rows are the
    colinear parts, reverse-strand rows the inversions.  DeviceQuery.segments equals
    rows_segments of the query's rows, and api.seq_kmer_segs the same."""
    torch = gpu
    from kmer_hasher_amd import api, device
    from kmer_hasher_amd.device import DeviceIndex
    k = 31
    s, a = _spliced(4096 + 37, 211, k)
    rows = _oracle_rows(a, k, rc_host(s) if rc else s, k)
    want = segs_ref.segments(rows)
    assert 3 <= len(want) <= 40 and len(rows) > 900
    t = torch.from_numpy(s).cuda()
    idx = DeviceIndex.build(torch.from_numpy(a).cuda(), k)
    q = idx.query_rc(t, k) if rc else idx.query(t, k)
    for ml in (1, 2, 300):
        got = q.segments(ml)
        assert torch.equal(got, device.rows_segments(q.rows(), ml)), ml
        assert np.array_equal(got.cpu().numpy(), want[want[:, 2] >= ml]), ml
    assert np.array_equal(segs_ref.expand(q.segments().cpu().numpy()), rows)
    q.free()
    idx.free()
    ptr = api.make_kmer_hash(a, k)
    assert np.array_equal(api.seq_kmer_segs(ptr, s, k, min_len=2, rc=rc), want[want[:, 2] >= 2])
    ptr.free()


def test_runs_handle_is_refused_in_the_rows_entries_words(gpu):
    torch = gpu
    import ctypes as C
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd.device import DeviceIndex
    L = _lib.lib()
    s = synth.iid(5000, 9)                           # a self query: one run
    t = torch.from_numpy(s).cuda()
    idx = DeviceIndex.build(t, 31)
    q, h, nr = C.c_void_p(), C.c_int64(), C.c_int64()
    _lib.check(L.kmhg_query_run_device_range_runs(
        idx.handle, C.c_void_p(t.data_ptr()), t.numel(), 31, 0, t.numel() - 30, None,
        C.byref(q), C.byref(h), C.byref(nr)))
    assert nr.value >= 0                             # it holds runs
    g, n = C.c_void_p(), C.c_int64()
    assert L.kmhg_query_segments(q, 1, C.byref(g), C.byref(n)) == _lib.KMHG_EINVAL
    want = L.kmhg_last_error().decode()
    d = C.c_void_p()
    assert L.kmhg_query_rows_device(q, C.byref(d)) == _lib.KMHG_EINVAL
    assert want == L.kmhg_last_error().decode() and "runs" in want
    _lib.check(L.kmhg_query_free(q))
    idx.free()


def test_api_refuses_a_counts_index_and_passes_query_errors_on(gpu):
    from kmer_hasher_amd import api
    cp = api.count_kmers("ACGTACGTACGTAAACCC", (4, 0, 1))
    with pytest.raises(api.KmerHashError) as e:
        api.seq_kmer_segs(cp, "ACGTACGT", 4)
    assert str(e.value) == "segments need a position index"
    cp.free()
    ptr = api.make_kmer_hash("ACGTACGTACGTAAACCC", 4)
    with pytest.raises(api.KmerHashError) as e:
        api.seq_kmer_segs(ptr, "ACG", 4)
    assert str(e.value) == "the sequence should be longer than k and k should not be longer than 31"
    for ml in (0, -1):
        with pytest.raises(api.KmerHashError) as e:
            api.seq_kmer_segs(ptr, "ACGTACGT", 4, min_len=ml)
        assert str(e.value) == MINLEN
    got = api.seq_kmer_segs(ptr, "ACGTACGT", 4)
    assert got.shape[1] == 3 and got[:, 2].sum() == len(api.seq_kmer_pos(ptr, "ACGTACGT", 4))
    ptr.free()
