"""seq.kmer.blocks -- the diagonal segments of a seq.kmer.pos result merged across small gaps
(kmhg_rows_blocks / kmhg_query_blocks, kmhg_blocks.hip) -- against tests/blocks_ref.py, the numpy
restatement of the definition in include/kmhgpu.h, computed from crafted rows or from the
clean-room oracle's rows.  Integer work: every comparison is exact, order included.  The passes
run over tiles of 2,048 SEGMENTS, so the crafted shapes count segments, not rows."""
import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import blocks_ref
import segs_ref
from test_blocks_host import TESTFA_FIGURES, figures
from test_gpu_query_rc import _spliced

pytestmark = pytest.mark.gpu

M = 2**31 - 1
TILE = 2048


def _dev(torch, rows):
    r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 2))
    return torch.from_numpy(r).cuda()


def _blocks(torch, t, max_gap, min_len=1, min_hits=1):
    from kmer_hasher_amd import device
    got = device.rows_blocks(t, max_gap, min_len, min_hits)
    assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 4 and got.is_cuda
    return got.cpu().numpy()


def _check(torch, rows, params):
    """The device's blocks of `rows` against blocks_ref at every (max_gap, min_len, min_hits);
    returns the references."""
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    t = _dev(torch, rows)
    segs = segs_ref.segments(rows)
    out = []
    for max_gap, min_len, min_hits in params:
        want = blocks_ref.merge(segs[segs[:, 2] >= min_len], max_gap, min_hits)
        got = _blocks(torch, t, max_gap, min_len, min_hits)
        assert got.shape == want.shape and np.array_equal(got, want), \
            (len(rows), max_gap, min_len, min_hits)
        out.append(want)
    return out


def _diagonal_rows(lens, gaps, j0=1):
    """Rows of one diagonal (i, i + j0 - 1) whose segments have the given lengths, segment t + 1
    starting gaps[t] windows after the end of segment t."""
    i, rows = 1, []
    for t, n in enumerate(lens):
        rows.append(np.arange(i, i + n))
        i += n + (gaps[t] if t < len(gaps) else 0)
    i = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return np.stack([i, i + j0 - 1], axis=1)


# ------------------------------------------------------------------ 1. crafted rows
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_one_diagonal_of_singles(gpu, n):
    t = np.arange(n, dtype=np.int64)
    rows = np.stack([2 * t + 1, 2 * t + 1], axis=1)
    apart, joined, at_n, above_n, far = _check(
        gpu, rows, [(0, 1, 1), (1, 1, 1), (1, 1, max(n, 1)), (1, 1, n + 1), (2**40, 1, 1)])
    assert len(apart) == n and (n == 0 or (apart[:, 2:] == 1).all())
    if n:                                            # the last n: a block longer than a tile
        assert joined.tolist() == at_n.tolist() == far.tolist() == [[1, 1, 2 * n - 1, n]]
    assert len(above_n) == 0


def test_two_interleaved_diagonals(gpu):
    """(2t + 1, 2t + 1) and (2t + 1, 2t + 6): the diagonal order is not the row order."""
    n = TILE + 5
    t = np.arange(n, dtype=np.int64)
    i = np.repeat(2 * t + 1, 2)
    j = np.stack([2 * t + 1, 2 * t + 6], axis=1).reshape(-1)
    apart, joined = _check(gpu, np.stack([i, j], axis=1), [(0, 1, 1), (1, 1, 1)])
    assert len(apart) == 2 * n
    assert joined.tolist() == [[1, 1, 2 * n - 1, n], [1, 6, 2 * n - 1, n]]


def test_alternating_gaps(gpu):
    n = 2 * TILE + 5
    rows = _diagonal_rows([1] * n, [1 if t % 2 == 0 else 3 for t in range(n - 1)], j0=3)
    got = _check(gpu, rows, [(g, 1, 1) for g in (0, 1, 2, 3)] + [(1, 1, 2), (1, 2, 1)])
    assert [len(b) for b in got] == [n, (n + 1) // 2, (n + 1) // 2, 1, n // 2, 0]
    assert got[3].tolist() == [[1, 3, int(rows[-1, 0]), n]]


def test_min_len_bridge_across_a_tile_boundary(gpu):
    """Lengths 3, 1, 3, 1, ... with gaps of 1: min_len = 2 drops the singles, and the gap between
    their kept neighbours, 1 + 1 + 1, spans them.  2,050 segments are kept of 4,099."""
    n = 2 * TILE + 3
    rows = _diagonal_rows([3 if t % 2 == 0 else 1 for t in range(n)], [1] * (n - 1))
    kept = TILE + 2
    bridged, apart, unfiltered, none = _check(
        gpu, rows, [(3, 2, 1), (2, 2, 1), (1, 1, 1), (2**40, 4, 1)])
    assert bridged.tolist() == [[1, 1, 6 * kept - 3, 3 * kept]]
    assert len(apart) == kept and (apart[:, 2:] == 3).all()
    assert unfiltered.tolist() == [[1, 1, 6 * kept - 3, 4 * kept - 1]]
    assert len(none) == 0


def test_extreme_coordinates(gpu):
    ext = [(1, 1), (2, 2), (M - 1, M - 1), (M, M)]
    apart, joined, any_gap, beyond = _check(
        gpu, ext, [(M - 5, 1, 1), (M - 4, 1, 1), (M - 2, 1, 1), (2**40, 1, 1)])
    assert apart.tolist() == [[1, 1, 2, 2], [M - 1, M - 1, 2, 2]]
    assert joined.tolist() == any_gap.tolist() == beyond.tolist() == [[1, 1, M, 4]]
    _check(gpu, [(1, 1), (1, M), (M, 1), (M, M)], [(0, 1, 1), (M, 1, 1), (M - 2, 1, 2)])
    _check(gpu, [(1, M - 1), (2, M), (M - 1, 1), (M, 2)], [(0, 1, 1), (2**40, 2, 2)])


def test_refusals_carry_their_words_and_the_library_goes_on(gpu):
    torch = gpu
    from kmer_hasher_amd import _lib, device
    L = _lib.lib()

    def refused(rows, args, msg):
        t = torch.tensor(rows, dtype=torch.int32, device="cuda").reshape(-1, 2)
        with pytest.raises(RuntimeError) as e:
            device.rows_blocks(t, *args)
        assert L.kmhg_last_error().decode() == msg and msg in str(e.value)

    good = [(1, 1), (2, 2), (4, 4)]
    for rows in (good, []):                          # also with no rows
        refused(rows, (1, 0, 1), "min_len must be a positive integer")
        refused(rows, (-1, 1, 1), "max_gap must not be negative")
        refused(rows, (1, 1, 0), "min_hits must be a positive integer")
        refused(rows, (-1, 0, 0), "min_len must be a positive integer")
    refused([(2, 2), (1, 1), (3, 3)], (1,), "rows are not in ascending (i, j) order")
    refused([(1, 1), (2, 2), (2, 2)], (1,), "rows are not in ascending (i, j) order")
    refused([(0, 1), (1, 2)], (1,), "rows must have i, j >= 1")
    assert _blocks(torch, _dev(torch, good), 1).tolist() == [[1, 1, 4, 3]]
    assert _blocks(torch, _dev(torch, good), 0).tolist() == [[1, 1, 2, 2], [4, 4, 1, 1]]


def test_runs_handle_is_refused_in_the_segments_entrys_words(gpu):
    torch = gpu
    import ctypes as C
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd.device import DeviceIndex
    L = _lib.lib()
    s = synth.iid(5000, 9)
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
    assert L.kmhg_query_blocks(q, 1, 0, 1, C.byref(g), C.byref(n)) == _lib.KMHG_EINVAL
    assert want == L.kmhg_last_error().decode() and "runs" in want
    _lib.check(L.kmhg_query_free(q))
    idx.free()


# ------------------------------------------------------------------ 2. oracle rows
def _oracle_rows(index_seq, k, query_seq, kq):
    return O.OracleIndex(index_seq, k).query(query_seq, kq).reshape(-1, 2)


def _substituted(seed):
    """A = synth.iid(6,200) and B = A with the base at every 100th position replaced by another
    one, plus one more 10 bases after position 3,000: at k = 31 an isolated substitution removes
    31 windows from the diagonal and the close pair 41.  Checked on the CPU: every row of the
    oracle lies on the main diagonal (no chance hit), so the blocks are derivable."""
    from kmer_hasher_amd import synth
    k = 31
    A = synth.iid(6200, seed)
    B = A.copy()
    subs = list(range(100, len(A), 100)) + [3010]
    for p in subs:
        B[p] = ord("ACGT"[("ACGT".index(chr(B[p])) + 1) % 4])
    rows = _oracle_rows(A.tobytes(), k, B.tobytes(), k)
    assert (rows[:, 1] - rows[:, 0] == rows[0, 1] - rows[0, 0]).all(), "chance hit: other seed"
    gaps = (len(subs) - 2) * [k] + [k + 10]
    return A, B, k, rows, gaps


def test_whole_route_with_a_derivable_answer(gpu):
    torch = gpu
    from kmer_hasher_amd import api, device
    from kmer_hasher_amd.device import DeviceIndex
    A, B, k, rows, gaps = _substituted(5)
    span = len(B) - k + 1
    i0, j0 = (int(x) for x in rows[0])
    segs = segs_ref.segments(rows)
    assert len(segs) == len(gaps) + 1 and len(rows) == span - sum(gaps)
    want = {30: np.column_stack([segs, segs[:, 2]]),
            31: blocks_ref.blocks(rows, 31),
            41: np.array([[i0, j0, span, span - sum(gaps)]], np.int32)}
    assert len(want[31]) == 2 and want[31][:, 2].sum() == span - 41     # apart at the close pair
    assert np.array_equal(blocks_ref.blocks(rows, 41), want[41])
    ptr = api.make_kmer_hash(A.tobytes(), k)
    idx = DeviceIndex.build(torch.from_numpy(A).cuda(), k)
    q = idx.query(torch.from_numpy(B).cuda(), k)
    for max_gap, w in want.items():
        a = api.seq_kmer_blocks(ptr, B.tobytes(), k, max_gap)
        b = q.blocks(max_gap).cpu().numpy()
        c = device.rows_blocks(q.rows(), max_gap).cpu().numpy()
        assert a.dtype == np.int32 and np.array_equal(a, w), max_gap
        assert np.array_equal(b, w) and np.array_equal(c, w), max_gap
    assert np.array_equal(api.seq_kmer_segs(ptr, B.tobytes(), k), segs)
    assert np.array_equal(api.seq_kmer_blocks(ptr, B.tobytes(), k), want[31])   # max_gap = k
    assert api.seq_kmer_blocks(ptr, B.tobytes(), k, min_hits=2100).tolist() == want[31][1:].tolist()
    q.free()
    idx.free()
    ptr.free()


def test_inverted_stretches_on_the_reverse_strand(gpu):
    torch = gpu
    from kmer_hasher_amd import api, device
    from kmer_hasher_amd.device import DeviceIndex
    k = 31
    s, a = _spliced(4096 + 37, 211, k)
    rows = _oracle_rows(a, k, rc_host(s), k)
    assert len(rows) > 900
    idx = DeviceIndex.build(torch.from_numpy(a).cuda(), k)
    q = idx.query_rc(torch.from_numpy(s).cuda(), k)
    ptr = api.make_kmer_hash(a, k)
    for max_gap, min_len, min_hits in ((0, 1, 1), (k, 1, 1), (2**31, 2, 300)):
        want = blocks_ref.blocks(rows, max_gap, min_len, min_hits)
        got = q.blocks(max_gap, min_len, min_hits)
        assert torch.equal(got, device.rows_blocks(q.rows(), max_gap, min_len, min_hits))
        assert np.array_equal(got.cpu().numpy(), want), (max_gap, min_len, min_hits)
        assert np.array_equal(api.seq_kmer_blocks(ptr, s, k, max_gap, min_len, min_hits, rc=True),
                              want)
    q.free()
    idx.free()
    ptr.free()


@pytest.fixture(scope="module")
def fa(testfa):
    """test.fa[:6000], k = 15, self: the oracle's rows and the reference segments, once."""
    s = testfa[:6000]
    rows = _oracle_rows(s, 15, s, 15)
    return dict(s=s, rows=rows, segs=segs_ref.segments(rows))


@pytest.fixture(scope="module")
def fa_rows(gpu, fa):
    return _dev(gpu, fa["rows"])


@pytest.mark.parametrize("max_gap,min_len,min_hits", list(TESTFA_FIGURES))
def test_testfa_self(gpu, fa, fa_rows, max_gap, min_len, min_hits):
    segs = fa["segs"]
    want = blocks_ref.merge(segs[segs[:, 2] >= min_len], max_gap, min_hits)
    got = _blocks(gpu, fa_rows, max_gap, min_len, min_hits)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert figures(got) == TESTFA_FIGURES[(max_gap, min_len, min_hits)]
    again = _blocks(gpu, fa_rows, max_gap, min_len, min_hits)      # determinism: identical bytes
    assert got.tobytes() == again.tobytes()


def test_segments_are_unchanged_beside_blocks(gpu, fa, fa_rows):
    from kmer_hasher_amd import device
    for ml in (1, 2):
        want = fa["segs"][fa["segs"][:, 2] >= ml]
        assert np.array_equal(device.rows_segments(fa_rows, ml).cpu().numpy(), want)


def test_api_refuses_a_counts_index_and_bad_parameters(gpu):
    from kmer_hasher_amd import api
    cp = api.count_kmers("ACGTACGTACGTAAACCC", (4, 0, 1))
    with pytest.raises(api.KmerHashError) as e:
        api.seq_kmer_blocks(cp, "ACGTACGT", 4)
    assert str(e.value) == "blocks need a position index"
    cp.free()
    ptr = api.make_kmer_hash("ACGTACGTACGTAAACCC", 4)
    for kw, msg in ((dict(min_len=0), "min_len must be a positive integer"),
                    (dict(max_gap=-1), "max_gap must not be negative"),
                    (dict(min_hits=0), "min_hits must be a positive integer")):
        with pytest.raises(api.KmerHashError) as e:
            api.seq_kmer_blocks(ptr, "ACGTACGT", 4, **kw)
        assert str(e.value) == msg
    got = api.seq_kmer_blocks(ptr, "ACGTACGT", 4)
    assert got.shape[1] == 4 and got[:, 3].sum() == len(api.seq_kmer_pos(ptr, "ACGTACGT", 4))
    ptr.free()
