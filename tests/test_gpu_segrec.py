"""The row-free seq.kmer.segs / seq.kmer.blocks (kmhg_segments_run_device, kmhg_blocks_run_device;
kmhg_segrec.hip): segments and blocks straight from a probed query's per-window records, no row
written.  The checker is tests/segs_ref.py / tests/blocks_ref.py on the clean-room oracle's rows;
wherever the rows route accepts the rows, DeviceQuery.segments() / .blocks() of the same query must
give the same bytes.  Integer work: every comparison is exact, order included.  The kernels walk
tiles of 2,048 WINDOWS, deal windows of more than 4 hits to the workgroup 256 hits a step, and
look one window back and one ahead, so the shapes sit around those numbers."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import blocks_ref
import segs_ref

pytestmark = pytest.mark.gpu

M = 2**31 - 1
TILE = 2048
BLOCK = 256
EMIT_DIRECT = 4


def _text(s):
    return s if isinstance(s, str) else np.asarray(s, np.uint8).tobytes().decode("latin-1")


def _seq_t(torch, s):
    a = np.frombuffer(s.encode("latin-1"), np.uint8) if isinstance(s, str) else s
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _index(torch, s, k):
    from kmer_hasher_amd.device import DeviceIndex
    return DeviceIndex.build(_seq_t(torch, s), k)


def _oracle_rows(a, k, q, kq, rc=False):
    q = _text(q)
    return O.OracleIndex(_text(a), k).query(rc_host(q) if rc else q, kq).reshape(-1, 2)


def _check(torch, idx, q, kq, rc, rows, min_lens=(1, 2), blocks=((0, 1, 1),), rows_route=True):
    """Both row-free entries on query q against the references of `rows` (the oracle's rows of the
    same query), and against the rows route of the same query; returns the reference segments."""
    t = _seq_t(torch, q)
    segs = segs_ref.segments(rows)
    dq = (idx.query_rc(t, kq) if rc else idx.query(t, kq)) if rows_route else None
    assert dq is None or dq.n_rows == len(rows)
    for ml in min_lens:
        got, h = idx.segments(t, kq, ml, rc=rc)
        assert h == len(rows), (h, len(rows))
        assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 3 and got.is_cuda
        want = segs[segs[:, 2] >= ml]
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (ml, rc)
        if dq is not None:
            assert torch.equal(got, dq.segments(ml)), (ml, rc)
    for max_gap, ml, mh in blocks:
        got, h = idx.blocks(t, kq, max_gap, ml, mh, rc=rc)
        assert h == len(rows)
        assert got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 4 and got.is_cuda
        want = blocks_ref.merge(segs[segs[:, 2] >= ml], max_gap, mh)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), \
            (max_gap, ml, mh, rc)
        if dq is not None:
            assert torch.equal(got, dq.blocks(max_gap, ml, mh)), (max_gap, ml, mh, rc)
    if dq is not None:
        dq.free()
    return segs


# ------------------------------------------------------------------ 1. test.fa self, both strands
@pytest.fixture(scope="module")
def fa(testfa):
    """test.fa[:6000], k = 15, self: the oracle's rows of either strand, once."""
    s = testfa[:6000]
    ox = O.OracleIndex(s, 15)
    fwd = ox.query(s, 15).reshape(-1, 2)
    rev = ox.query(rc_host(s), 15).reshape(-1, 2)
    assert len(fwd) == 5_275_316
    return s, fwd, rev


@pytest.mark.parametrize("rc", [False, True])
def test_testfa_self(gpu, fa, rc):
    s, fwd, rev = fa
    idx = _index(gpu, s, 15)
    params = [(g, 1, mh) for g in (0, 15, 2**31 - 2) for mh in (1, 50)]
    segs = _check(gpu, idx, s, 15, rc, rev if rc else fwd, (1, 2, 16), params)
    if not rc:
        assert len(segs) == 53_933
    idx.free()


# ------------------------------------------------------------------ 2. window-count boundaries
COUNTS = [1, 2, EMIT_DIRECT, EMIT_DIRECT + 1, BLOCK - 1, BLOCK + 1, TILE + 52]


@pytest.fixture(scope="module")
def counted_index():
    """Each unit (k + 5 chars: 6 windows) repeated c times, copies separated by N: a query window
    of the unit has exactly c hits."""
    k = 15
    rng = np.random.default_rng(123)
    units = ["".join(rng.choice(list("ACGT"), k + 5)) for _ in COUNTS]
    a = "".join((u + "N") * c for u, c in zip(units, COUNTS))
    return k, units, a, O.OracleIndex(a, k)


@pytest.mark.parametrize("nw", [TILE - 1, TILE, TILE + 1])
def test_window_counts(gpu, counted_index, nw):
    from kmer_hasher_amd import synth
    k, units, a, ox = counted_index
    head = "N".join(units) + "N"
    tail = "N" + units[3] + units[6][:k]             # hits in the last windows too
    L = nw + k - 1
    q = head + synth.iid(L - len(head) - len(tail), 900 + nw).tobytes().decode() + tail
    assert len(q) == L
    rows = ox.query(q, k).reshape(-1, 2)
    per_window = np.unique(rows[:, 0], return_counts=True)[1]
    assert set(COUNTS) <= set(per_window.tolist())
    assert rows[-1, 0] == L                          # the last window hits
    idx = _index(gpu, a, k)
    _check(gpu, idx, q, k, False, rows, (1, 6), [(0, 1, 1), (k, 1, 1), (k, 2, 7)])
    idx.free()


# ------------------------------------------------------------------ 3. shifted edges
def test_shifted_edges(gpu):
    """One query -- inverted stretches, N runs, lower case -- against an index that holds two
    stretches twice and one three times, behind p characters N: every diagonal crosses lane (64),
    wave-row (256) and tile (2,048) edges at some p, with multi-hit windows next to single-hit
    ones.  Both strands."""
    from kmer_hasher_amd import synth
    k = 15
    s = synth.iid(5000, 41)
    a = s.copy()
    for lo, ln in ((400, 500), (1700, 333), (3000, 640)):
        a[lo:lo + ln] = rc_host(s[lo:lo + ln])
    a = np.concatenate([a, a[1000:1400], a[1200:1300], a[2040:2060]])
    q = s.copy()
    q[200:260] = np.frombuffer(q[200:260].tobytes().lower(), np.uint8)
    q[1100:1103] = ord("N")
    q[2047] = ord("n")
    q[4000:4100] = ord("N")
    a, q = _text(a), _text(q)
    idx = _index(gpu, a, k)
    ox = O.OracleIndex(a, k)
    for p in (0, 1, 63, 64, 2047, 2048):
        qq = "N" * p + q
        for rc in (False, True):
            rows = ox.query(rc_host(qq) if rc else qq, k).reshape(-1, 2)
            assert len(rows) > 800
            if not rc:
                assert (np.unique(rows[:, 0], return_counts=True)[1] == 3).any()
            _check(gpu, idx, qq, k, rc, rows, (1, 2), [(0, 1, 1), (k, 1, 1), (2**31 - 2, 2, 2)])
    idx.free()


# ------------------------------------------------------------------ 4. lists as neighbours
@pytest.mark.parametrize("s,k,n_rows,n_segs", [
    ("ACGT" * 600, 5, 1_435_204, 1_197),             # different lists of nearly equal length
    ("A" * 3000, 15, 2986 * 2986, 2 * 2986 - 1),     # the same list
    ("A" * 1000 + "C" * 1000 + "A" * 500, 15, None, None)],   # list-to-none, list-to-list
    ids=["ACGT600", "A3000", "A1000C1000A500"])
def test_lists_as_neighbours(gpu, s, k, n_rows, n_segs):
    rows = _oracle_rows(s, k, s, k)
    idx = _index(gpu, s, k)
    segs = _check(gpu, idx, s, k, False, rows, (1, 3), [(0, 1, 1), (k, 1, 1), (k, 2, 9)])
    if n_rows is not None:
        assert (len(rows), len(segs)) == (n_rows, n_segs)
    idx.free()


# ------------------------------------------------------------------ 5. other shapes
def test_query_k_differs_from_index_k(gpu):
    """Index k = 12, query k = 15: a 15-mer's key equals a 12-mer's where its first three bases
    are A (code 0), so the rows are what the tables say and nothing a sequence comparison would
    give; runs of A make windows with many hits.  Every segment is what the rows say."""
    from kmer_hasher_amd import synth
    s = synth.iid(3000, 77)
    s[500:520] = ord("A")
    s[1500:1600] = ord("A")
    s = _text(s)
    rows = _oracle_rows(s, 12, s, 15)
    assert len(rows) > 3000 and np.unique(rows[:, 0], return_counts=True)[1].max() > BLOCK // 4
    idx = _index(gpu, s, 12)
    _check(gpu, idx, s, 15, False, rows, (1, 2), [(0, 1, 1), (15, 1, 1)])
    rows = _oracle_rows(s, 12, s, 15, rc=True)
    _check(gpu, idx, s, 15, True, rows, (1,), [(15, 1, 2)])
    idx.free()


def test_no_hit_one_window_and_two_calls(gpu):
    torch = gpu
    from kmer_hasher_amd import synth
    a = synth.iid(3000, 17)
    q = "T" * 3000
    assert len(_oracle_rows(a, 15, q, 15)) == 0
    idx = _index(torch, a, 15)
    for rc in (False, True):
        g, h = idx.segments(_seq_t(torch, q), 15, rc=rc)
        assert h == 0 and tuple(g.shape) == (0, 3)
        b, h = idx.blocks(_seq_t(torch, q), 15, 15, rc=rc)
        assert h == 0 and tuple(b.shape) == (0, 4)
    # one window (L == k + 1 is the shortest query the entries take: L must exceed k)
    one = _text(a[100:116])
    rows = _oracle_rows(a, 15, one, 15)
    assert len(rows) >= 1
    _check(torch, idx, one, 15, False, rows)
    # two calls: identical bytes
    s = "ACGT" * 300 + _text(a[:900])
    idx2 = _index(torch, s, 5)
    t = _seq_t(torch, s)
    a1, h1 = idx2.segments(t, 5)
    a2, h2 = idx2.segments(t, 5)
    b1, _ = idx2.blocks(t, 5, 5, 2, 3)
    b2, _ = idx2.blocks(t, 5, 5, 2, 3)
    assert h1 == h2 and a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes()
    assert len(b1) and b1.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes()
    idx.free()
    idx2.free()


# ------------------------------------------------------------------ 6., 7. beyond 2^31 / 2^32 rows
def _homopolymer_segments(n, k):
    """Index and query "A" * n at k: every one of nw = n - k + 1 windows hits all nw positions.
    In (i, j) order: (k, j, nw - j + 1) for j = 1..nw, then (i, 1, n - i + 1) for i = k + 1..n."""
    nw = n - k + 1
    j = np.arange(1, nw + 1, dtype=np.int64)
    i = np.arange(k + 1, n + 1, dtype=np.int64)
    top = np.stack([np.full(nw, k), j, nw - j + 1], axis=1)
    left = np.stack([i, np.ones(len(i), np.int64), n - i + 1], axis=1)
    return np.concatenate([top, left]).astype(np.int32)


def test_more_than_2_31_rows(gpu):
    """ "A" * 47000 against itself at k = 15: 46,986 windows of 46,986 hits each, 2,207,684,196
    rows -- which kmhg_query_segments refuses as "bad row count" -- and 93,971 segments, one per
    diagonal, in closed form.  Every window is dealt to its workgroup, and only 23 workgroups
    have work.  Measured on an MI355X: 2.14 s for the three calls and their checks (about 0.7 s a call)."""
    torch = gpu
    n, k = 47000, 15
    nw = n - k + 1
    s = "A" * n
    idx = _index(torch, s, k)
    t = _seq_t(torch, s)
    t0 = time.perf_counter()
    want = _homopolymer_segments(n, k)
    got, h = idx.segments(t, k)
    assert h == nw * nw == 2_207_684_196 and h > 2**31
    assert len(want) == 2 * nw - 1 == 93_971
    assert np.array_equal(got.cpu().numpy(), want)
    got, h = idx.segments(t, k, 40000)
    assert h == nw * nw and np.array_equal(got.cpu().numpy(), want[want[:, 2] >= 40000])
    got, h = idx.blocks(t, k, k)
    assert h == nw * nw
    assert np.array_equal(got.cpu().numpy(), np.column_stack([want, want[:, 2]]))
    print(f"beyond 2^31 rows: {time.perf_counter() - t0:.2f} s for three calls")
    idx.free()


def test_more_than_2_32_rows_blocks(gpu):
    """ "A" * 66000 at k = 15: H = 65,986^2 = 4,354,152,196 > 2^32, so the block passes' len
    prefixes wrap; every block is one segment and its hits, a difference of two prefixes modulo
    2^32, must equal its span.  Measured on an MI355X: 1.00 s for the call and its check."""
    torch = gpu
    n, k = 66000, 15
    nw = n - k + 1
    s = "A" * n
    idx = _index(torch, s, k)
    t = _seq_t(torch, s)
    t0 = time.perf_counter()
    got, h = idx.blocks(t, k, k)
    assert h == nw * nw == 4_354_152_196 and h > 2**32
    got = got.cpu().numpy()
    want = _homopolymer_segments(n, k)
    assert np.array_equal(got[:, 3], got[:, 2])
    assert np.array_equal(got, np.column_stack([want, want[:, 2]]))
    print(f"beyond 2^32 rows: {time.perf_counter() - t0:.2f} s")
    idx.free()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_their_words_and_order(gpu):
    torch = gpu
    from kmer_hasher_amd import _lib, api, synth
    from kmer_hasher_amd.device import DeviceIndex
    L = _lib.lib()
    s = synth.iid(5000, 9)
    t = torch.from_numpy(s).cuda()
    idx = DeviceIndex.build(t, 31)
    ERR = "the sequence should be longer than k and k should not be longer than 31"

    def segs(h, seq=t, n=None, k=31, min_len=1, out=True, code=_lib.KMHG_EINVAL):
        g, ns, nr = C.c_void_p(), C.c_int64(), C.c_int64()
        rc = L.kmhg_segments_run_device(
            h, C.c_void_p(seq.data_ptr()) if seq is not None else None,
            t.numel() if n is None else n, k, 0, min_len, None, C.byref(g) if out else None,
            C.byref(ns), C.byref(nr))
        assert rc == code
        return L.kmhg_last_error().decode()

    def blks(h, seq=t, n=None, k=31, min_len=1, max_gap=0, min_hits=1, out=True,
             code=_lib.KMHG_EINVAL):
        g, nb, nr = C.c_void_p(), C.c_int64(), C.c_int64()
        rc = L.kmhg_blocks_run_device(
            h, C.c_void_p(seq.data_ptr()) if seq is not None else None,
            t.numel() if n is None else n, k, 0, min_len, max_gap, min_hits, None,
            C.byref(g) if out else None, C.byref(nb), C.byref(nr))
        assert rc == code
        return L.kmhg_last_error().decode()

    part = DeviceIndex.build_part(t, 31, 0, 2)
    cp = api.count_kmers("ACGTACGTACGTAAACCC", (4, 0, 1))
    sh = api.count_kmers_fq_sh_rp("no-such-file.fq", [15, 10, 0, 1, -1, 1, 1, 0])
    h = idx.handle
    # each refusal with every later fault present too: the earlier word wins
    assert segs(None, min_len=0, k=32) == "null argument"
    assert segs(h, seq=None, min_len=0) == "null argument"
    assert segs(h, out=False, min_len=0) == "null argument"
    assert segs(part.handle, min_len=0, k=32) == "min_len must be a positive integer"
    assert segs(part.handle, k=32) == ERR
    assert segs(part.handle, k=0) == ERR
    assert segs(part.handle, n=31) == ERR
    assert segs(h, n=2**31 - 1, code=_lib.KMHG_EOVERFLOW) == \
        "sequence longer than 2^31-1 (int positions)"
    assert segs(part.handle) == "a part index must be assembled before it is queried"
    assert segs(cp.handle, k=4) == "segments need a position index"
    assert segs(sh.handle, k=15) == "External pointer has incorrect tag"
    assert blks(None, min_len=0) == "null argument"
    assert blks(h, seq=None, max_gap=-1) == "null argument"
    assert blks(h, out=False, min_hits=0) == "null argument"
    assert blks(part.handle, min_len=0, max_gap=-1, min_hits=0, k=32) == \
        "min_len must be a positive integer"
    assert blks(part.handle, max_gap=-1, min_hits=0, k=32) == "max_gap must not be negative"
    assert blks(part.handle, min_hits=0, k=32) == "min_hits must be a positive integer"
    assert blks(part.handle, k=32) == ERR
    assert blks(part.handle, n=31) == ERR
    assert blks(part.handle) == "a part index must be assembled before it is queried"
    assert blks(cp.handle, k=4) == "blocks need a position index"
    assert blks(sh.handle, k=15) == "External pointer has incorrect tag"
    cp.free()
    sh.free()
    # the wrappers raise the same words
    with pytest.raises(_lib.KmhgError, match="min_len must be a positive integer"):
        idx.segments(t, 31, 0)
    with pytest.raises(_lib.KmhgError, match="max_gap must not be negative"):
        idx.blocks(t, 31, -1)
    # min_len / min_hits beyond int32 are legal and keep nothing; and the library goes on
    g, n = idx.segments(t, 31, 2**40)
    assert n == 4970 and len(g) == 0
    b, n = idx.blocks(t, 31, 0, 1, 2**40)
    assert n == 4970 and len(b) == 0
    g, n = idx.segments(t, 31)
    assert n == 4970 and g.cpu().numpy().tolist() == [[31, 1, 4970]]
    b, n = idx.blocks(t, 31, 2**40)
    assert b.cpu().numpy().tolist() == [[31, 1, 4970, 4970]]


# ------------------------------------------------------------------ 9. host API
def test_host_api_row_free_equals_the_rows_route(gpu, testfa):
    from kmer_hasher_amd import api
    s = testfa[:6000]
    ptr = api.make_kmer_hash(s, 15)
    # (the reverse strand of this telomeric stretch has few hits or none: equality is the check)
    for rc in (False, True):
        a = api.seq_kmer_segs(ptr, s, 15, rc=rc)
        b = api.seq_kmer_segs(ptr, s, 15, rc=rc, row_free=True)
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)
        assert rc or len(a) == 53_933
        assert np.array_equal(api.seq_kmer_segs(ptr, s, 15, 16, rc=rc),
                              api.seq_kmer_segs(ptr, s, 15, 16, rc=rc, row_free=True))
        for kw in (dict(), dict(max_gap=0), dict(max_gap=100, min_len=2, min_hits=50)):
            a = api.seq_kmer_blocks(ptr, s, 15, rc=rc, **kw)
            b = api.seq_kmer_blocks(ptr, s, 15, rc=rc, row_free=True, **kw)
            assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b)
            assert rc or len(a) > 0, kw
    # validation is the same on either route
    cp = api.count_kmers("ACGTACGTACGTAAACCC", (4, 0, 1))
    for rf in (False, True):
        with pytest.raises(api.KmerHashError) as e:
            api.seq_kmer_segs(cp, "ACGTACGT", 4, row_free=rf)
        assert str(e.value) == "segments need a position index"
        with pytest.raises(api.KmerHashError) as e:
            api.seq_kmer_blocks(cp, "ACGTACGT", 4, row_free=rf)
        assert str(e.value) == "blocks need a position index"
        for fn, kw, msg in ((api.seq_kmer_segs, dict(min_len=0), "min_len must be a positive integer"),
                            (api.seq_kmer_blocks, dict(max_gap=-1), "max_gap must not be negative"),
                            (api.seq_kmer_blocks, dict(min_hits=0),
                             "min_hits must be a positive integer")):
            with pytest.raises(api.KmerHashError) as e:
                fn(ptr, s, 15, row_free=rf, **kw)
            assert str(e.value) == msg
        with pytest.raises(api.KmerHashError, match="should be longer than k"):
            api.seq_kmer_segs(ptr, "ACGT", 15, row_free=rf)
    cp.free()
    ptr.free()
