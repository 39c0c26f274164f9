"""seq.kmer.pos.rc -- the query's reverse complement against the index, staged on the device from
the forward sequence (kmhg_query_run_rc*, k_query_probe<..., RC>) -- against the clean-room
oracle queried with tests/revcomp_ref.py's rc_host of the same string: the definition in
include/kmhgpu.h says the result is exactly the forward query of rc(S).  Integer work: every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host

pytestmark = pytest.mark.gpu

ERR = "the sequence should be longer than k and k should not be longer than 31"


def _want(index_seq, k, query_seq, kq):
    return O.OracleIndex(index_seq, k).query(rc_host(query_seq), kq)


def _rows(q):
    r = q.rows().cpu().numpy().reshape(-1)
    q.free()
    return r


# ------------------------------------------------------------------ 1. edge strings, exact rows
EDGE = [("ACGTA", 3), ("ACGTNACG", 3), ("ACGTNACGT", 3),
        ("ACGNTTTT", 3),            # an initial segment of exactly k, then N: dropped on rc only
        ("TTTTNACG", 3), ("acgtNNacgt", 2), ("AAAAAA", 2), ("NNNNNNNN", 3),
        ("ACGTRYKMSWBDHV-." * 4, 3), ("ACGT", 3)]                      # ... and L = k + 1


@pytest.mark.parametrize("s,k", EDGE)
def test_edge_strings_exact_rows(gpu, s, k):
    from kmer_hasher_amd import api
    for index_seq in (s, rc_host(s), "ACGTTGCAACGTNACGTAAAATTTT"):
        if len(index_seq) <= k or set(index_seq.upper()) <= {"N"}:
            continue
        ptr = api.make_kmer_hash(index_seq, k)
        got = api.seq_kmer_pos_rc(ptr, s, k)
        assert got.dtype == np.int32 and got.shape[1] == 2
        assert np.array_equal(got.reshape(-1), _want(index_seq, k, s, k)), (s, index_seq)
        ptr.free()


def test_end_drop_quirk_is_not_mirror_symmetric(gpu):
    """"ACGNTTTT" at k = 3: forward, the initial ACG is a window; on the reverse strand it is the
    final N-free segment of exactly k chars and the reference's walk drops it."""
    from kmer_hasher_amd import api
    ptr = api.make_kmer_hash("CGTACGT", 3)           # holds CGT = rc(ACG)
    assert api.seq_kmer_pos(ptr, "ACGNTTTT", 3).shape[0] > 0
    assert api.seq_kmer_pos_rc(ptr, "ACGNTTTT", 3).shape[0] == 0
    assert api.seq_kmer_pos_rc(ptr, "ACGTNTTTT", 3).shape[0] > 0      # k + 1 chars: kept
    assert np.array_equal(api.seq_kmer_pos_rc(ptr, "NNNNNNNN", 3), np.empty((0, 2), np.int32))
    ptr.free()


def test_errors_are_the_forward_entrys(gpu):
    from kmer_hasher_amd import api
    ptr = api.make_kmer_hash("ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", 3)
    for s, k in (("ACG", 3), ("AC", 3), ("ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", 32),
                 ("ACGTA", 0)):
        with pytest.raises(api.KmerHashError) as e:
            api.seq_kmer_pos_rc(ptr, s, k)
        assert str(e.value) == ERR
        with pytest.raises(api.KmerHashError) as e:
            api.seq_kmer_pos(ptr, s, k)
        assert str(e.value) == ERR
    ptr.free()


# ------------------------------------------------------------------ 2. every residue of L mod 16
def _spliced(n, seed, k):
    """iid sequence and an index sequence of it with 3 inverted segments of 300-700 chars."""
    from kmer_hasher_amd import synth
    s = synth.iid(n, seed)
    a = s.copy()
    rng = np.random.default_rng(seed)
    for lo in (400, 1700, 3000):
        ln = int(rng.integers(300, 701))
        a[lo:lo + ln] = rc_host(s[lo:lo + ln])
    return s, a


@pytest.mark.parametrize("r", range(16))
def test_every_residue_of_length_aligned_and_unaligned_pointer(gpu, r):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    k = 31
    L = 4096 + 30 + r
    s, a = _spliced(L, 100 + r, k)
    idx = DeviceIndex.build(torch.from_numpy(a).cuda(), k)
    want = _want(a, k, s, k)
    assert len(want) > 2 * 300                       # the inverted segments hit
    t = torch.from_numpy(s).cuda()
    assert t.data_ptr() % 16 == 0
    assert np.array_equal(_rows(idx.query_rc(t, k)), want), ("aligned", r)
    for off in (1, 7):
        buf = torch.zeros(L + 32, dtype=torch.uint8, device="cuda")
        v = buf[off:off + L]
        v.copy_(t)
        assert v.data_ptr() % 16 == off
        assert np.array_equal(_rows(idx.query_rc(v, k)), want), (off, r)
    idx.free()


# ------------------------------------------------------------------ 3. tile boundaries
@pytest.mark.parametrize("n", [40, 2047 + 30, 2048 + 30, 2049 + 30, 3 * 2048 + 7])
def test_tile_boundaries(gpu, n):
    from kmer_hasher_amd import api
    rng = np.random.default_rng(77 + n)
    s = "".join(rng.choice(list("ACGT"), n))
    a = s[: n // 2] + rc_host(s[n // 2:])
    ptr = api.make_kmer_hash(a, 8)
    oi = O.OracleIndex(a, 8)
    for kq in (8, 6):
        want = oi.query(rc_host(s), kq)
        assert len(want) > 0 or kq != 8             # (another k: the keys rarely coincide)
        assert np.array_equal(api.seq_kmer_pos_rc(ptr, s, kq).reshape(-1), want), (n, kq)
    ptr.free()


# ------------------------------------------------------------------ 4. paths
_AB = {}


def _ab():
    """A (300 K iid with N-runs, k = 21), B = derived(A) with inversions, and the oracle's
    expectations, computed once."""
    if not _AB:
        from kmer_hasher_amd import synth
        A = synth.add_n_runs(synth.iid(300_000, 61), 0.0005, 62, max_run=40)
        B = synth.derived(A, 63)
        U = synth.iid(120_000, 64)
        oi = O.OracleIndex(A, 21)
        _AB.update(A=A, B=B, U=U, oi=oi,
                   want_B=oi.query(rc_host(B), 21), fwd_B=oi.query(B, 21),
                   want_A=oi.query(A, 21),                  # query rc(A) on the reverse strand
                   want_U=oi.query(rc_host(U), 21))
    return _AB


HEAVY = "AC" * 3000 + "ACGTTGCA" * 500 + "A" * 5000


@pytest.mark.parametrize("path", ["default", "nodiag", "notags"])
def test_paths_vs_oracle(gpu, test_lib, monkeypatch, path):
    torch = gpu
    from kmer_hasher_amd import api
    from kmer_hasher_amd.device import DeviceIndex
    if path == "nodiag":
        monkeypatch.setenv("KMHG_QUERY_DIAG", "0")
    elif path == "notags":
        monkeypatch.setenv("KMHG_QUERY_TAGS", "0")
    d = _ab()
    k = 21
    idx = DeviceIndex.build(torch.from_numpy(d["A"]).cuda(), k)
    # B holds inversions of A: rows the forward strand lacks
    got_B = _rows(idx.query_rc(torch.from_numpy(d["B"]).cuda(), k))
    assert np.array_equal(got_B, d["want_B"])
    fwd_j = set(map(tuple, d["fwd_B"].reshape(-1, 2).tolist()))
    L = d["B"].size
    rc_as_fwd = {(L - i + k, j) for i, j in got_B.reshape(-1, 2).tolist()}   # same window's end
    assert len(got_B) > 2 * 1000 and len(rc_as_fwd - fwd_j) > 1000
    # A's own reverse complement as the query, read on the reverse strand: every window hits
    rcA = torch.from_numpy(rc_host(d["A"])).cuda()
    got_A = _rows(idx.query_rc(rcA, k))
    assert np.array_equal(got_A, d["want_A"]) and len(got_A) // 2 >= idx.info()["n_positions"]
    # unrelated: every window misses
    got_U = _rows(idx.query_rc(torch.from_numpy(d["U"]).cuda(), k))
    assert np.array_equal(got_U, d["want_U"]) and len(got_U) == 0
    idx.free()
    # more rows than windows: the emit's redo into an exact buffer
    ptr = api.make_kmer_hash(rc_host(HEAVY), 6)
    want = O.OracleIndex(rc_host(HEAVY), 6).query(rc_host(HEAVY), 6)
    got = api.seq_kmer_pos_rc(ptr, HEAVY, 6)
    assert got.shape[0] > 2 * len(HEAVY)
    assert np.array_equal(got.reshape(-1), want)
    ptr.free()


# ------------------------------------------------------------------ 5. ranges
@pytest.mark.parametrize("case", ["tiles", "B"])
def test_ranges_concatenate_and_runs_expand(gpu, case):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex, runs_expand
    if case == "tiles":
        k = 8
        rng = np.random.default_rng(5)
        n = 3 * 2048 + 7
        s = np.frombuffer("".join(rng.choice(list("ACGT"), n)).encode(), np.uint8).copy()
        a = np.concatenate([s[: n // 2], rc_host(s[n // 2:])])
        want = _want(a, k, s, k)
    else:
        d = _ab()
        k, a, s, want = 21, d["A"], d["B"], d["want_B"]
    idx = DeviceIndex.build(torch.from_numpy(a).cuda(), k)
    t = torch.from_numpy(s).cuda()
    nw = s.size - k + 1
    cuts = [0, 1, 2047, 2048, 2049, nw - 1, nw]
    parts = []
    for w0, w1 in zip(cuts[:-1], cuts[1:]):
        rows = _rows(idx.query_range_rc(t, k, w0, w1))
        kind, rt, h = idx.query_range_runs_rc(t, k, w0, w1)
        assert h == len(rows) // 2, (w0, w1)
        if kind == "runs":
            out = torch.empty((h, 2), dtype=torch.int32, device="cuda")
            runs_expand(rt, h, out)
            got = out.cpu().numpy().reshape(-1)
        else:
            got = rt.cpu().numpy().reshape(-1)
        assert np.array_equal(got, rows), (case, w0, w1, kind)
        parts.append(rows)
    assert np.array_equal(np.concatenate(parts), want)
    assert np.array_equal(_rows(idx.query_range_rc(t, k, 0, nw)), want)
    assert idx.query_range_rc(t, k, 5, 5).n_rows == 0
    idx.free()


# ------------------------------------------------------------------ 6. counts index
def test_counts_index_rows_equal_forward_on_rc(gpu):
    from kmer_hasher_amd import api
    seqs = ["ACGTACGTTTNACGTACGAGGGACGTACG", "TTTACGNACGTCCGGAAT"]
    ptr = api.count_kmers([seqs[0]], (4, 0, 2))
    api.count_kmers([seqs[1]], (4, 1, 2), ptr)
    for s in seqs + ["ACGTNCGTACGTAAACG"]:
        got = api.seq_kmer_pos_rc(ptr, s, 4)
        assert got.shape[0] > 0
        assert np.array_equal(got, api.seq_kmer_pos(ptr, rc_host(s), 4)), s
    ptr.free()


# ------------------------------------------------------------------ 7. refusals
def test_refusals(gpu):
    torch = gpu
    from kmer_hasher_amd import _lib, synth
    from kmer_hasher_amd.device import DeviceIndex
    seq = torch.from_numpy(synth.iid(50_000, 35)).cuda()
    p = DeviceIndex.build_part(seq, 21, 0, 2)
    for call in (lambda: p.query_rc(seq, 21), lambda: p.query_range_rc(seq, 21, 0, 100),
                 lambda: p.query_range_runs_rc(seq, 21, 0, 100)):
        with pytest.raises(_lib.KmhgError, match="a part index must be assembled before it is queried"):
            call()
    p.free()
    idx = DeviceIndex.build(seq, 21)
    L = _lib.lib()
    q, h, nr = C.c_void_p(), C.c_int64(), C.c_int64()
    sp = C.c_void_p(seq.data_ptr())
    assert L.kmhg_query_run_rc(None, b"ACGTACGT", 8, 3, C.byref(q), C.byref(h)) == _lib.KMHG_EINVAL
    assert L.kmhg_query_run_rc(idx.handle, None, 8, 3, C.byref(q), C.byref(h)) == _lib.KMHG_EINVAL
    assert L.kmhg_query_run_rc(idx.handle, b"ACGTACGT", 8, 3, None, C.byref(h)) == _lib.KMHG_EINVAL
    assert L.kmhg_query_run_rc_device_range(idx.handle, None, 50_000, 21, 0, 10, None,
                                            C.byref(q), C.byref(h)) == _lib.KMHG_EINVAL
    assert L.kmhg_query_run_rc_device_range_runs(None, sp, 50_000, 21, 0, 10, None, C.byref(q),
                                                 C.byref(h), C.byref(nr)) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error() == b"null argument"
    with pytest.raises(_lib.KmhgError, match="window range out of bounds"):
        idx.query_range_rc(seq, 21, 0, 50_000)
    idx.free()


# ------------------------------------------------------------------ 8. forward unchanged
def test_forward_query_of_b_still_equals_the_oracle(gpu):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    d = _ab()
    idx = DeviceIndex.build(torch.from_numpy(d["A"]).cuda(), 21)
    assert np.array_equal(_rows(idx.query(torch.from_numpy(d["B"]).cuda(), 21)), d["fwd_B"])
    idx.free()
