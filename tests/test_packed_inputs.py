"""The packed-read generators of tests/packed_inputs.py reach the kernel branches they claim
(conditions on the offsets, as the kernels compute them), and the two sources of expected values
agree on these inputs: fq_walk with the compiled reference's walk (sh1), oracle.read_kmers with
the compiled reference's iterator and reader (rp).  CPU only; the comparisons with the compiled
reference are skipped when oracle/_ref is not built."""
import ctypes as C

import numpy as np
import pytest

import fq_sh_inputs as I
import fq_walk as W
import packed_inputs as P
import ref_fq_sh as R
from oracle import oracle as O

needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libkmh_ref_sh.so not built")
LEADS = (0, 5, 16, 4099)


@pytest.mark.parametrize("k", P.KS)
def test_ragged_batches_reach_their_branches(k):
    seed = P.SEEDS[k]
    for n in P.N_READS:
        for share in P.SHARES:
            recs, seq, qual, off, hasq = P.ragged_batch(seed, k, n, share)
            assert len(recs) == n <= 300 and off[-1] <= 300_000
            assert len(seq) == len(qual) == off[-1] + 16
            assert not seq[off[-1]:].any() and not qual[off[-1]:].any()
            assert set(np.diff(off).tolist()) <= set(P.lengths(k))
            assert hasq.all() if share == 0 else not hasq.any() if share == 1 else True
            assert not qual[np.repeat(hasq == 0, np.diff(off)).nonzero()[0]].any()
            assert len(P.wave_spans(off)) == (n + P.RK_READS - 1) // P.RK_READS
    for share in P.SHARES:
        recs, seq, qual, off, hasq = P.ragged_batch(seed, k, 200, share)
        spans = P.wave_spans(off)
        assert (spans > P.RK_CAP).any() and (spans <= P.RK_CAP).any()      # both walks of a wave
        assert (P.wave_bases(off) % 16 != 0).any()
        ln = np.diff(off)
        assert set(ln.tolist()) == set(P.lengths(k))                       # every length drawn
        if share:
            assert 0 < (hasq == 0).sum() and P.lanes_with_multiple_records(off, hasq).max() >= 3
        body = seq[:off[-1]]
        assert 0.01 < ((body | 0x20) == ord("n")).mean() < 0.03
        # the four NULs: first byte, last byte, middle, directly after a full init window
        at = sorted((int(p - off[r]), int(ln[r]))
                    for p in np.flatnonzero(body == 0)
                    for r in [int(np.searchsorted(off, p, side="right")) - 1])
        assert len(at) == 4
        assert any(p == 0 for p, n in at) and any(p == n - 1 for p, n in at)
        assert any(p == n // 2 for p, n in at) and any(p == k for p, n in at)


@pytest.mark.parametrize("variant", list(P.SUB_VARIANTS))
@pytest.mark.parametrize("k", P.KS)
def test_sub_range_batches_start_where_they_claim(k, variant):
    rem, before, first, a = P.SUB_VARIANTS[variant]
    (recs, seq, qual, off, hasq), i0, i1 = P.sub_range_batch(P.SEEDS[k], k, variant)
    assert len(recs) <= 300 and off[-1] <= 300_000 and 0 < i0 < i1 < len(recs)
    assert off[i0] % 16 == rem and off[i0] > 0
    if variant.startswith("below16"):
        assert 0 < off[i0] < 16
    b = seq[off[i0] - 1]
    assert {"nul": b == 0, "n": b == ord("N"), "plain": b in b"ACGT"}[before]
    assert P.fa_tile_origin(off[i0:i1 + 1]) == off[i0] - rem
    assert (P.wave_bases(off[i0:i1 + 1])[0] % 16 != 0) == (rem != 0)
    assert (i1 - i0) % P.RK_READS and i0 % P.RK_READS
    assert off[i0 + 1] - off[i0] == {"fastq_150": 150, "fasta_k1": k + 1, "fasta_k": k,
                                     "fastq_k": k}[first]
    assert bool(hasq[i0]) == first.startswith("fastq")
    # the neighbour's tail and the first record's head would make a window if read across
    if before == "plain" and a:
        assert all(c in b"ACGT" for c in seq[off[i0] - k:off[i0] + k].tobytes())


@pytest.mark.parametrize("final_extra", (0, 1))
@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("k", P.KS)
def test_fa_tile_batch_marks_sit_on_the_tile_arithmetic(k, lead, final_extra):
    (recs, seq, qual, off, hasq), m = P.fa_tile_batch(k, lead, final_extra)
    T = I.FA_TILE
    assert len(recs) <= 300 and off[-1] <= 300_000 and not hasq.any() and not qual.any()
    assert off[1] == lead
    sub = off[1:]
    t0 = P.fa_tile_origin(sub)
    assert t0 == m["t0"] == lead - lead % 16
    # record 1 spans three tiles and holds the Ns around both inner tile edges
    assert (off[1] - t0) // T == 0 and (off[2] - 1 - t0) // T == 2
    assert sorted((p - t0) % T for p in m["n_pos"]) == sorted([T - 1, 0, T - (k - 1)] * 2)
    for p in m["n_pos"] + [m["final_n"]]:
        assert off[1] <= p < off[2] and seq[p] == ord("N")
    body = seq[off[1]:off[2]]
    assert int(np.flatnonzero(body == ord("N")).max()) == len(body) - (k + final_extra) - 1
    # the run: lengths 0 .. k + 2, several records in one lane, one across the tile edge
    r0, r1 = m["run"]
    assert r1 - r0 == 48 and set(np.diff(off[r0:r1 + 1]).tolist()) == set(range(k + 3))
    assert (m["run_edge"] - t0) % T == 0
    assert any(off[r] < m["run_edge"] < off[r + 1] for r in range(r0, r1))
    lanes = P.lanes_with_multiple_records(sub, hasq[1:])
    assert lanes[(int(off[r0]) - t0) // P.FA_CPT] >= 3
    # the NUL on a tile edge, inside the last record
    assert seq[m["nul_pos"]] == 0 and (m["nul_pos"] - t0) % T == 0
    assert off[-2] < m["nul_pos"] < off[-1] - 1 and (seq[:off[-1]] == 0).sum() == 1


def _generated(k):
    """Every generated record of one k: the ragged batch, the sub-ranges' crafted records, the
    tile batches."""
    recs = list(P.ragged_batch(P.SEEDS[k], k, 200, 1 / 3)[0])
    for v, (_, _, _, a) in P.SUB_VARIANTS.items():
        recs += P.sub_range_batch(P.SEEDS[k], k, v)[0][0][a:a + 2]
    return recs


@pytest.mark.parametrize("k", P.KS)
def test_vectorised_keys_equal_fq_walk(k):
    """packed_inputs.sh1_keys is fq_walk.record_keys; records of length <= k yield nothing."""
    recs = _generated(k) + list(P.fa_tile_batch(k, 5, 1)[0][0][3:])
    short = 0
    for s, q in recs:
        want = W.record_keys(s, q, k, I.MQ)
        assert P.sh1_keys((s, q), k).tolist() == want
        if len(s) <= k:
            short += 1
            assert want == []
    assert short >= 20


@needs_ref
@pytest.mark.parametrize("k", P.KS)
def test_fq_walk_equals_reference_walk(k):
    """fq_walk.record_keys against seq_to_counts_sh over the compiled init_kmer_qual_2
    (ref_fq_sh.RefSH1.add_record): the keys of every record longer than k, and the counts of all."""
    recs = [r for r in _generated(k) if len(r[0]) > k]
    for lead in LEADS[1:3]:
        recs += [r for r in P.fa_tile_batch(k, lead, 0)[0][0] if len(r[0]) > k]
    ref = R.RefSH1(k, I.prefix_bits_for(k))
    per = []
    for s, q in recs:
        ref.keys = set()
        ref.add_record(s, q, I.MQ)
        mine = P.sh1_keys((s, q), k)
        assert set(mine.tolist()) == ref.keys
        per.append(mine)
    keys, cnt = P.table_of_keys(per)
    ref.keys = set(keys.tolist())
    rk, rc = ref.arrays()
    assert len(keys) > 1000 and np.array_equal(rk, keys) and np.array_equal(rc, cnt)
    ref.close()


def _ref_iterator_keys(L, s, q, k, min_q):
    """The compiled reference's own kmer_iterator (src/kmer_util.c:55-162) over one string."""
    it = C.create_string_buffer(256)                   # kmer_iterator: 80 bytes
    L.kmer_iterator_init(it, C.c_uint32(k), C.c_ubyte((33 + min_q) & 0xFF))
    f, r = C.c_uint64(), C.c_uint64()
    out = []
    ok = L.kmer_iterator_begin(it, s, q, C.byref(f), C.byref(r))
    while ok:
        out.append(min(f.value, r.value))
        ok = L.kmer_iterator_next(it, C.byref(f), C.byref(r))
    return out


@needs_ref
@pytest.mark.parametrize("k", P.KS)
def test_read_kmers_equals_reference_iterator(k):
    """oracle.read_kmers against the reference's iterator called on each string as it is, records
    of length <= k included (a record of exactly k bases yields its one window: the <= k filter is
    the reader's, not the iterator's); then over a FASTX file against the reference's reader, for
    the records it keeps."""
    L = R.lib()
    for fn in (L.kmer_iterator_begin, L.kmer_iterator_next):
        fn.restype = C.c_int
    recs = _generated(k)
    exact_k = 0
    for s, q in recs + [(s, None) for s, q in recs if q is not None]:
        got = O.read_kmers(s, q, k, P.MQ_RP).tolist()
        assert got == _ref_iterator_keys(L, s, q, k, P.MQ_RP)
        if len(s) == k and b"N" not in s.upper() and q is None:
            exact_k += 1
            assert len(got) == 1
        if len(s) < k:
            assert got == []
    assert exact_k >= 3


@needs_ref
@pytest.mark.parametrize("k", P.KS)
def test_read_kmers_equals_reference_reader(k, tmp_path):
    # FASTA records first: after a FASTQ record the reference hands a FASTA record stale
    # qualities (tests/sh_inputs.py tricky_fastx); NUL-free, as a file's records are
    recs = P.ragged_records(P.SEEDS[k], k, 200, 1 / 3, nuls=False)
    recs = [r for r in recs if r[1] is None] + [r for r in recs if r[1] is not None]
    p = str(tmp_path / "ragged.fx")
    with open(p, "wb") as f:
        f.write(I.fastx_bytes(recs))
    kept = [r for r in O.fastx_records(O.read_fastx(p)) if len(r[0]) > k]
    assert kept == [r for r in recs if len(r[0]) > k]
    keys, cnt = P.table_of_keys([P.rp_keys(r, k) for r in kept])
    ref = O.RefSH().add_fastq(p, k, min(8, 2 * k), P.MQ_RP, 2**62, 1, 0)
    rk, rm = ref.arrays()
    assert len(keys) > 1000 and np.array_equal(rk, keys) and np.array_equal(rm[:, 0], cnt)
    ref.close()
