"""reads.kmer.pos / reads.kmer.vote on the device (kmhg_readsq.hip) against tests/reads_ref.py: the
oracle's single query read by read and strand by strand, and a dictionary count for the vote.
Integer work: every comparison is exact, order included."""
import os

import numpy as np
import pytest

from maxocc_ref import TILE
from oracle import oracle as O
from reads_ref import pack, rows_ref, votes_ref
from revcomp_ref import rc_host

pytestmark = pytest.mark.gpu

KS = (5, 15, 31)
BANDS = (1, 7, 64, 2**30)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _index_seq():
    """6,000 bases with a 40-copy repeat planted (copies apart, so its windows hit 40 times) and
    a palindromic stretch (its own reverse complement) at 3,000."""
    rng = np.random.default_rng(20240)
    a = _ACGT[rng.integers(0, 4, 6000)]
    unit = _ACGT[rng.integers(0, 4, 45)]
    for c in range(40):
        a[200 + 60 * c:200 + 60 * c + 45] = unit
    half = _ACGT[rng.integers(0, 4, 40)]
    a[3000:3080] = np.concatenate([half, rc_host(half)])
    return a.tobytes().decode()


A = _index_seq()
_OX = {}


def _ox(k):
    if k not in _OX:
        _OX[k] = O.OracleIndex(A, k)
    return _OX[k]


def _cut(rng, lo, n, strand=1, sub=0.02):
    s = np.frombuffer(A[lo:lo + n].encode(), np.uint8).copy()
    m = rng.random(n) < sub
    s[m] = _ACGT[rng.integers(0, 4, int(m.sum()))]
    return (s if strand == 1 else rc_host(s)).tobytes().decode()


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _real_reads(rng, n, length=150):
    out = []
    for i in range(n):
        if i % 5 == 4:
            out.append(_rand(rng, length))                       # unrelated
        else:
            out.append(_cut(rng, int(rng.integers(0, len(A) - length)), length,
                            1 if i % 2 == 0 else -1))
    return out


def _dev(torch, reads):
    seq, off = pack(reads)
    return torch.from_numpy(seq).cuda(), torch.from_numpy(off).cuda()


@pytest.fixture(scope="module")
def indexes(gpu):
    from kmer_hasher_amd.device import DeviceIndex
    a = gpu.from_numpy(np.frombuffer(A.encode(), np.uint8).copy()).cuda()
    made = {k: DeviceIndex.build(a, k).wait() for k in KS}
    yield made
    for ix in made.values():
        ix.free()


def _run(torch, ix, reads, k, strands=3):
    q = ix.query_reads(_dev(torch, reads), k, strands)
    rows = q.rows().cpu().numpy()
    assert rows.shape == (q.n_rows, 4) and rows.dtype == np.int32
    return q, rows


def _check(torch, ix, reads, k, index_k=None, strands=3, max_occ=0, bands=()):
    index_k = index_k or k
    want = rows_ref(A, index_k, reads, k, strands, max_occ, _ox(index_k))
    q, rows = _run(torch, ix, reads, k, strands)
    assert np.array_equal(rows, want), (k, strands, rows.shape, want.shape)
    for band in bands:
        got = q.votes(band).cpu().numpy()
        assert np.array_equal(got, votes_ref(want, len(reads), k, band)), band
    q.free()
    return want


@pytest.mark.parametrize("k", KS)
def test_lengths_n_case_and_codes(gpu, indexes, k):
    rng = np.random.default_rng(k)
    body = _cut(rng, 500, 150)
    reads = [_cut(rng, 1000, n) for n in (0, 1, k - 1, k, k + 1, 150)]
    reads += [body[:60] + "N" + body[60:60 + k],          # ends in N + k bases: window dropped
              body[:k] + "N" + body[k:90],                # starts with k bases, then N: its mirror
              "N" * 40, "n" * (k + 1),
              _cut(rng, 2000, 150).lower(),
              body[:50] + "RYKMSWBDHV-." + body[62:],
              _cut(rng, 230, 120, -1), _rand(rng, 150), ""]
    want = _check(gpu, indexes[k], reads, k, bands=BANDS)
    assert want.shape[0] > 0
    assert {1, -1} <= set(want[:, 1].tolist())


@pytest.mark.parametrize("strands", (1, 2, 3))
def test_strands(gpu, indexes, strands):
    rng = np.random.default_rng(7)
    want = _check(gpu, indexes[15], _real_reads(rng, 12), 15, strands=strands, bands=(64,))
    assert set(want[:, 1].tolist()) == {1: {1}, 2: {-1}, 3: {1, -1}}[strands]


@pytest.mark.parametrize("edge", (TILE - 1, TILE, TILE + 1))
def test_read_boundary_at_tile_edge(gpu, indexes, edge):
    """Forward only, so a base is an entry of the batch: the first read ends where entry `edge`
    begins, and the batch has more than one tile."""
    rng = np.random.default_rng(edge)
    reads = [_cut(rng, 100, 1500), _cut(rng, 1700, edge - 1500, -1), _cut(rng, 4000, 150),
             _cut(rng, 4100, 150, -1)]
    _check(gpu, indexes[15], reads, 15, strands=1)
    _check(gpu, indexes[15], reads, 15, strands=3, bands=(64,))


@pytest.mark.parametrize("total", (TILE, TILE + 1, 2 * TILE + 1))
@pytest.mark.parametrize("strands", (1, 3))
def test_batch_of_exactly_n_entries(gpu, indexes, total, strands):
    """A batch of exactly `total` entries (strands = 1: bases; both strands: two per base)."""
    rng = np.random.default_rng(total)
    bases = total if strands == 1 else (total + 1) // 2
    reads = _real_reads(rng, bases // 150)
    reads.append(_cut(rng, 300, bases - 150 * (bases // 150)))
    assert sum(map(len, reads)) == bases
    _check(gpu, indexes[15], reads, 15, strands=strands)


def test_thousands_of_tiny_reads_in_one_tile(gpu, indexes):
    """5,000 reads of one to three bases and 3,000 empty ones (more offsets than a tile stages),
    none with a window, then real reads."""
    rng = np.random.default_rng(11)
    reads = [_rand(rng, int(rng.integers(1, 4))) for _ in range(5000)]
    reads[1000:1000] = [""] * 3000
    reads += _real_reads(rng, 6)
    want = _check(gpu, indexes[5], reads, 5, bands=(64,))
    assert want[:, 0].min() > 8000


def test_one_long_read_between_short_ones(gpu, indexes):
    rng = np.random.default_rng(12)
    long_read = _cut(rng, 900, 2 * TILE + 300)
    reads = _real_reads(rng, 3) + [long_read] + _real_reads(rng, 3)
    for strands in (1, 2, 3):
        _check(gpu, indexes[31], reads, 31, strands=strands, bands=(7,))


def test_exact_redo_when_rows_exceed_the_guess(gpu):
    from kmer_hasher_amd.device import DeviceIndex
    idx_seq = "A" * 3000
    ix = DeviceIndex.build(gpu.from_numpy(np.frombuffer(idx_seq.encode(), np.uint8).copy()).cuda(),
                           15).wait()
    reads = ["A" * 200] * 3
    want = rows_ref(idx_seq, 15, reads, 15, 3)
    q, rows = _run(gpu, ix, reads, 15)
    assert rows.shape[0] > 2 * 3 * 200 * 2          # far beyond one row per entry
    assert np.array_equal(rows, want)
    assert np.array_equal(q.votes(64).cpu().numpy(), votes_ref(want, 3, 15, 64))
    q.free()
    ix.free()


def test_max_occ(gpu, indexes):
    rng = np.random.default_rng(13)
    reads = [_cut(rng, 200, 150), _cut(rng, 380, 150, -1)] + _real_reads(rng, 4)
    ix = indexes[15]
    free = rows_ref(A, 15, reads, 15, 3, 0, _ox(15))
    ix.set_max_occ(8)
    try:
        capped = _check(gpu, ix, reads, 15, max_occ=8, bands=(64,))
    finally:
        ix.set_max_occ(0)
    assert 0 < capped.shape[0] < free.shape[0]


def test_query_k_differs_from_index_k(gpu, indexes):
    rng = np.random.default_rng(14)
    want = _check(gpu, indexes[15], _real_reads(rng, 6) + ["ACGTACG"], 9, index_k=15)
    assert want.shape[0] > 0


def test_two_runs_give_identical_bytes(gpu, indexes):
    rng = np.random.default_rng(15)
    reads = _real_reads(rng, 20) + [_cut(rng, 200, 400)]
    q1, r1 = _run(gpu, indexes[15], reads, 15)
    q2, r2 = _run(gpu, indexes[15], reads, 15)
    assert r1.tobytes() == r2.tobytes()
    assert q1.votes(7).cpu().numpy().tobytes() == q2.votes(7).cpu().numpy().tobytes()
    q1.free()
    q2.free()


def test_votes_ties_no_hit_and_nonpositive_pos(gpu, indexes):
    from kmer_hasher_amd.device import rows_votes
    rng = np.random.default_rng(16)
    k = 15
    pal = A[3000:3080]                                # its own reverse complement: a strand tie
    assert rc_host(pal) == pal
    near = "".join(_rand(rng, 30)) + A[:100]          # overhangs the index's start: pos <= 0
    reads = [pal, _rand(rng, 150), near, rc_host(near), _cut(rng, 200, 150)] + _real_reads(rng, 5)
    want = rows_ref(A, k, reads, k, 3, 0, _ox(k))
    assert ((want[:, 3] - want[:, 2] + k) <= 0).any()
    q, rows = _run(gpu, indexes[k], reads, k)
    assert np.array_equal(rows, want)
    shuffled = gpu.from_numpy(want[np.random.default_rng(1).permutation(want.shape[0])]).cuda()
    for band in BANDS:
        ref = votes_ref(want, len(reads), k, band)
        assert np.array_equal(q.votes(band).cpu().numpy(), ref), band
        assert np.array_equal(rows_votes(shuffled, len(reads), k, band).cpu().numpy(), ref), band
    ref = votes_ref(want, len(reads), k, 64)
    assert ref[0, 1] == 1 and ref[0, 3] == ref[0, 4] > 0      # the tie went to the forward strand
    assert tuple(ref[1]) == (2, 0, 0, 0, 0, 0)
    q.free()


def test_reads_handle_route_matches_packed_route(gpu, tmp_path):
    """kmhg_fastx_read + kmhg_reads_query_run on a FASTQ file against the packed route on the same
    records: the reference's test_10.fastq (which shares 8-mers but no 15-mer with test.fa), and
    reads cut from test.fa on both strands, with an empty record, so the index's own k has rows."""
    from kmer_hasher_amd import api
    here = os.path.dirname(os.path.abspath(__file__))
    idx_seq = "".join(l.strip() for l in open(os.path.join(here, "golden", "test.fa"))
                      if not l.startswith(">"))
    ptr = api.make_kmer_hash(idx_seq, 15)
    ox = O.OracleIndex(idx_seq, 15)
    rng = np.random.default_rng(19)
    cut = []
    for i in range(12):
        lo = int(rng.integers(0, len(idx_seq) - 150))
        r = idx_seq[lo:lo + int(rng.integers(10, 150))]
        cut.append(r if i % 2 == 0 else rc_host(r))
    cut[5] = ""                                      # an empty record: dropped by the reader
    made = tmp_path / "cut.fastq"
    made.write_text("".join(f"@r{i}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(cut)))
    golden = os.path.join(here, "golden", "test_10.fastq")
    for path, ks in ((str(made), (15,)), (golden, (8,))):
        recs = [s.decode() for s, _ in O.fastx_records(O.read_fastx(path))]
        recs = [r for r in recs if r]                # read numbers are the non-empty records'
        for k in ks:
            by_file = api.reads_kmer_pos(ptr, path, k)
            by_list = api.reads_kmer_pos(ptr, recs, k)
            assert by_file.shape[0] > 0 and np.array_equal(by_file, by_list), (path, k)
            assert np.array_equal(by_list, rows_ref(idx_seq, 15, recs, k, ox=ox))
            assert path == golden or {1, -1} <= set(by_file[:, 1].tolist())
            assert np.array_equal(api.reads_kmer_vote(ptr, path, k, 7),
                                  votes_ref(by_list, len(recs), k, 7))
    assert len([r for r in cut if r]) == 11
    ptr.free()


def test_device_reads_input(gpu, indexes):
    """DeviceReads (padded bases, its own n_bases) through query_reads, against the pair route."""
    from kmer_hasher_amd.device import DeviceReads
    rng = np.random.default_rng(20)
    reads = _real_reads(rng, 9, 100)
    arr = np.frombuffer("".join(reads).encode(), np.uint8).reshape(9, 100)
    dr = DeviceReads.from_arrays(arr, np.full_like(arr, ord("I")), "cuda")
    assert dr.seq.numel() > dr.n_bases == 900
    want = rows_ref(A, 15, reads, 15, 3, 0, _ox(15))
    q = indexes[15].query_reads(dr, 15)
    assert want.shape[0] > 0 and np.array_equal(q.rows().cpu().numpy(), want)
    assert np.array_equal(q.votes(64).cpu().numpy(), votes_ref(want, 9, 15, 64))
    q.free()


def test_bad_offsets_through_the_device_entry(gpu, indexes):
    """An off that decreases once, and one whose last entry is not the number of bases: the device
    raises its flag, the call returns KMHG_EINVAL, and the next query runs.  Every off here keeps
    every read it describes inside the buffer."""
    from kmer_hasher_amd import _lib
    rng = np.random.default_rng(17)
    reads = _real_reads(rng, 8)
    seq, off = _dev(gpu, reads)
    down = off.clone()
    down[3] = down[2] - 10
    short = off.clone()
    short[-1] -= 5
    for bad in (down, short):
        with pytest.raises(_lib.KmhgError) as e:
            indexes[15].query_reads((seq, bad), 15)
        assert e.value.code == _lib.KMHG_EINVAL
        assert "non-decreasing" in str(e.value)
    # bases that no read holds: refused on the host, before the one-entry off is searched
    with pytest.raises(_lib.KmhgError) as e:
        indexes[15].query_reads((seq, gpu.zeros(1, dtype=gpu.int64, device="cuda")), 15)
    assert e.value.code == _lib.KMHG_EINVAL and "non-decreasing" in str(e.value)
    q = indexes[15].query_reads((seq[:0], gpu.zeros(1, dtype=gpu.int64, device="cuda")), 15)
    assert q.n_rows == 0 and q.votes(64).shape == (0, 6)
    q.free()
    _check(gpu, indexes[15], reads, 15)


def test_refusals_with_an_index_launch_nothing(gpu, indexes):
    """k, strands, and a minimizer-sampled index at its own k: refused with code and message
    (the sampled index at another k runs, as in seq.kmer.pos)."""
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex
    rng = np.random.default_rng(18)
    reads = _real_reads(rng, 4)
    dev = _dev(gpu, reads)
    for k, strands, text in ((0, 3, "k should be between 1 and 31"),
                             (32, 3, "k should be between 1 and 31"),
                             (15, 0, "strands must be 1 (forward), 2 (reverse) or 3 (both)"),
                             (15, 4, "strands must be 1 (forward), 2 (reverse) or 3 (both)")):
        with pytest.raises(_lib.KmhgError) as e:
            indexes[15].query_reads(dev, k, strands)
        assert e.value.code == _lib.KMHG_EINVAL and str(e.value) == text
    a = gpu.from_numpy(np.frombuffer(A.encode(), np.uint8).copy()).cuda()
    sampled = DeviceIndex.build(a, 15, w=4).wait()
    with pytest.raises(_lib.KmhgError) as e:
        sampled.query_reads(dev, 15)
    assert e.value.code == _lib.KMHG_EINVAL and "follow-up" in str(e.value)
    sampled.query_reads(dev, 9).free()
    sampled.free()


def test_counts_index_and_overflow_refusals(gpu, indexes):
    """A count.kmers index, and more bases or reads than a call takes: each refused with its code
    and message before anything is launched (the counts are far beyond the tensors passed)."""
    import ctypes as C
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex
    rng = np.random.default_rng(21)
    seq, off = _dev(gpu, _real_reads(rng, 4))
    a = gpu.from_numpy(np.frombuffer(A.encode(), np.uint8).copy()).cuda()
    counts = DeviceIndex.count(a, 15, 0, 1)
    with pytest.raises(_lib.KmhgError) as e:
        counts.query_reads((seq, off), 15)
    assert e.value.code == _lib.KMHG_EINVAL
    assert str(e.value) == "reads are queried against a position index, not a counts index"
    counts.free()
    L = _lib.lib()
    q, h = C.c_void_p(), C.c_int64()
    for n_bases, n_reads, text in (
            (2**31 - 1, 4, "more than 2^31-2 bases in one call: split the reads"),
            (600, 2**31, "more than 2^31-1 reads in one call: split the reads")):
        rc = L.kmhg_reads_query_run_device(indexes[15]._h, C.c_void_p(seq.data_ptr()), n_bases,
                                           C.c_void_p(off.data_ptr()), n_reads, 15, 3, None,
                                           C.byref(q), C.byref(h))
        assert rc == _lib.KMHG_EOVERFLOW and L.kmhg_last_error().decode() == text
        assert not q.value
