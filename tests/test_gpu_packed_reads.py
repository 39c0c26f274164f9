"""The device entries of read counting (kmhg_sh_count_reads_device: "rp", kmhg_sh1_count_reads_device:
"sh1") at the shapes tests/packed_inputs.py builds: ragged lengths from 0 to 5000 bases, record
arrays that do not start at offset 0, FASTA records against k_fa_kmers' tile edges, the host split
of sh_count_reads_host, and both branches of k_spectrum.  Every comparison is exact: the key-sorted
table against a Counter over per-record expected keys (fq_walk for sh1, oracle.read_kmers for rp;
neither needs oracle/_ref).  Each case asserts the host-side predicate of the branch it names.

Every record is walked as given (no <= k filter in the device entries): sh1 yields nothing for a
record of length <= k because the init window ends the record; rp yields what the reference's
iterator yields for that string, one window for an accepted record of exactly k bases."""
import ctypes as C

import numpy as np
import pytest

import fq_sh_inputs as I
import packed_inputs as P
from oracle import oracle as O

pytestmark = pytest.mark.gpu
WALKS = ("rp", "sh1")


def _table(ptr):
    from kmer_hasher_amd import api
    keys, M = api.counts_table(ptr)
    o = np.argsort(keys, kind="stable")
    return keys[o], (M[o, 0] if len(keys) else np.zeros(0, np.int32))


def _to_device(torch, batch):
    _, seq, qual, off, hasq = batch
    t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (seq, qual, off, hasq)]
    # the documented contract: 16-byte-aligned bases, >= 16 readable bytes past the last read
    assert t[0].data_ptr() % 16 == 0 and t[1].data_ptr() % 16 == 0
    assert len(seq) >= off[-1] + 16 and len(qual) == len(seq)
    return t


def _count(torch, walk, k, dev, i0, i1, ptr=None):
    """Records [i0, i1) of a device batch into ptr (a new hash when None): the base pointers of
    seq / qual stay, offsets and has_qual move by i0."""
    from kmer_hasher_amd import _lib, api
    ds, dq, do, dh = dev
    h = C.c_void_p(ptr.handle.value if ptr is not None else None)
    if walk == "sh1":
        prm = (C.c_int32 * 6)(*I.params(k))
        fn, tag = _lib.lib().kmhg_sh1_count_reads_device, api.SUFFIX_HASH_TAG
    else:
        prm = (C.c_int32 * 8)(k, 10, P.MQ_RP, 1, -1, 1, 1, 0)
        fn, tag = _lib.lib().kmhg_sh_count_reads_device, api.SUFFIX_HASH_N_TAG
    _lib.check(fn(C.byref(h), ds.data_ptr(), dq.data_ptr(), do.data_ptr() + 8 * i0,
                  dh.data_ptr() + i0, i1 - i0, prm, None))
    torch.cuda.synchronize()
    if ptr is not None:
        return ptr
    return api.ExtPtr(h.value, tag=tag) if h.value else None


def _assert_table(ptr, per_record):
    keys, cnt = P.table_of_keys(per_record)
    if ptr is None:                                   # nothing to count: no hash was made
        assert len(keys) == 0
        return
    gk, gc = _table(ptr)
    assert np.array_equal(gk, keys) and np.array_equal(gc, cnt)


@pytest.mark.parametrize("share3", (0, 1, 3))
@pytest.mark.parametrize("n", P.N_READS)
@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("walk", WALKS)
def test_ragged_whole_batch(gpu, walk, k, n, share3):
    """Lengths 0 .. 5000 in one batch.  Reaches: k_read_ub / k_sh1_ub with ub = 0 and ub = 1;
    k_rk_span and both walks of a wave (LDS-staged: span <= 28,672 B, global cursor: above) at
    n = 200; a last wave of 63 / 64 / 1 reads at n = 63, 64, 65; the route n_noq == 0
    (share 0: k_fa_kmers not launched), n_noq == n_reads (share 1: lane kernel not launched)
    and both kernels into one key stream (share 1/3); record_of and k_fa_kmers' record loop over
    empty and one-base records; k_sh1_nul at a record's first, last and middle byte."""
    batch = P.ragged_batch(P.SEEDS[k], k, n, share3 / 3)
    recs, seq, qual, off, hasq = batch
    ln = np.diff(off)
    assert len(P.wave_spans(off)) == (n + 63) // 64
    assert {0: hasq.all(), 1: 0 < hasq.sum() < n or n == 1, 3: not hasq.any()}[share3]
    if n == 200:
        spans = P.wave_spans(off)
        assert (spans > P.RK_CAP).any() and (spans <= P.RK_CAP).any()
        assert (P.wave_bases(off) % 16 != 0).any()
        assert (ln < k).any() and (ln == k).any() and (ln == 0).any()      # ub = 0, ub = 1
        assert (seq[:off[-1]] == 0).sum() == 4
        if share3:
            assert P.lanes_with_multiple_records(off, hasq).max() >= 3
    ptr = _count(gpu, walk, k, _to_device(gpu, batch), 0, n)
    _assert_table(ptr, P.record_keys_cached(walk, k, ("ragged", P.SEEDS[k], n, share3)))


@pytest.mark.parametrize("variant", list(P.SUB_VARIANTS))
@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("walk", WALKS)
def test_sub_range(gpu, walk, k, variant):
    """d_offsets + i0 with the batch's own base pointers, off[i0] = 16 m + {0, 1, 15} and
    0 < off[i0] < 16.  Reaches: the align-down of k_read_kmers / k_read_kmers_sh1 (base =
    off[r0] & ~15 below the first read), k_sh1_nul's and k_fa_kmers' clips (p < lo, max(p0, lo),
    `open` only for p > rb) with a NUL, an N or plain bases just before off[i0], and a stage
    that starts before the buffer (sb = -16, p >= 0) when off[i0] < 16."""
    rem, before, first, a = P.SUB_VARIANTS[variant]
    batch, i0, i1 = P.sub_range_batch(P.SEEDS[k], k, variant)
    _, seq, _, off, hasq = batch
    assert off[i0] % 16 == rem and off[i0] > 0 and i0 % 64 and (i1 - i0) % 64
    assert P.fa_tile_origin(off[i0:i1 + 1]) == off[i0] - rem
    assert (P.fa_tile_origin(off[i0:i1 + 1]) - 16 < 0) == variant.startswith("below16")
    b = seq[off[i0] - 1]
    assert {"nul": b == 0, "n": b == ord("N"), "plain": b in b"ACGT"}[before]
    assert bool(hasq[i0]) == first.startswith("fastq") and hasq[i0:i1].min() == 0
    ptr = _count(gpu, walk, k, _to_device(gpu, batch), i0, i1)
    per = P.record_keys_cached(walk, k, ("sub", P.SEEDS[k], variant))
    _assert_table(ptr, per[i0:i1])


@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("walk", WALKS)
def test_split_equals_whole(gpu, walk, k):
    """[0, n) in one call against [0, i0), [i0, i1), [i1, n) into one pointer, i0 and i1 at
    unaligned offsets: the calls sh_count_reads_host makes past 2^32 bases (absolute offsets,
    later batches merged into the existing table)."""
    batch, i0, i1 = P.sub_range_batch(P.SEEDS[k], k, "rem15_plain")
    off = batch[3]
    n = len(off) - 1
    while off[i1] % 16 == 0:
        i1 += 1
    assert off[i0] % 16 == 15 and off[i1] % 16 != 0 and i1 < n
    dev = _to_device(gpu, batch)
    whole = _count(gpu, walk, k, dev, 0, n)
    parts = _count(gpu, walk, k, dev, 0, i0)
    for a, b in ((i0, i1), (i1, n)):
        assert _count(gpu, walk, k, dev, a, b, parts) is parts
    wk, wc = _table(whole)
    pk, pc = _table(parts)
    assert np.array_equal(wk, pk) and np.array_equal(wc, pc)
    _assert_table(whole, P.record_keys_cached(walk, k, ("sub", P.SEEDS[k], "rem15_plain")))


@pytest.mark.parametrize("final_extra", (0, 1))
@pytest.mark.parametrize("lead", (0, 5, 16, 4099))
@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("walk", ("sh1", "rp_noq"))
def test_fa_tile_batch(gpu, walk, k, lead, final_extra):
    """FASTA records against k_fa_kmers' tiles, which start at (off[i0] & ~15) + 4096 j: an N on
    the last char of a tile, on the first, and k - 1 before the edge (the halo and `open` across
    tiles); a final N-free segment of exactly k (the window that opens its segment and ends the
    record: not counted) and of k + 1; 48 records of 0 .. k + 2 bases, four of them in one lane's
    16 starts and one across a tile edge (the lane's record loop, ub = 0 / 1); a NUL on a tile
    edge (k_sh1_nul, eend).  Counted as the sub-range [1, n) and whole.  rp_noq: the same bytes
    through kmhg_sh_count_reads_device with has_qual = 0, the N-only iterator of walk_read."""
    batch, m = P.fa_tile_batch(k, lead, final_extra)
    _, seq, _, off, hasq = batch
    n = len(off) - 1
    t0 = P.fa_tile_origin(off[1:])
    assert off[1] == lead and t0 == m["t0"] and not hasq.any()
    assert sorted((p - t0) % I.FA_TILE for p in m["n_pos"]) == \
        sorted([I.FA_TILE - 1, 0, I.FA_TILE - (k - 1)] * 2)
    assert all(seq[p] == ord("N") for p in m["n_pos"] + [m["final_n"]])
    assert off[2] - m["final_n"] - 1 == k + final_extra
    assert (m["nul_pos"] - t0) % I.FA_TILE == 0 and seq[m["nul_pos"]] == 0
    r0, r1 = m["run"]
    assert P.lanes_with_multiple_records(off[1:], hasq[1:])[(int(off[r0]) - t0) // 16] >= 3
    assert any(off[r] < m["run_edge"] < off[r + 1] for r in range(r0, r1))
    dev = _to_device(gpu, batch)
    per = P.record_keys_cached(walk, k, ("fa", lead, final_extra))
    w = "sh1" if walk == "sh1" else "rp"
    _assert_table(_count(gpu, w, k, dev, 1, n), per[1:])
    _assert_table(_count(gpu, w, k, dev, 0, n), per)


# ---------------------------------------------------------------- spectrum branches
SPEC_LDS_BINS = 8192            # kmhg_sh.hip: bins held in LDS when they fit


@pytest.mark.parametrize("mc", (8190, 8191, 8192, 10000))
def test_spectrum_sh1_lds_and_global_bins(gpu, mc):
    """kmer.spec.sh: max_count + 1 = 8,191 / 8,192 bins (k_spectrum's LDS branch) and 8,193 /
    10,001 (global atomics), from a repeat-rich hash (the ragged batch counted twice and its
    first half a third time: counts 2, 3 and multiples) read back with kmhg_counts_export."""
    from kmer_hasher_amd import api
    k = 21
    batch = P.ragged_batch(P.SEEDS[k], k, 200, 1 / 3)
    dev = _to_device(gpu, batch)
    ptr = _count(gpu, "sh1", k, dev, 0, 200)
    _count(gpu, "sh1", k, dev, 0, 200, ptr)
    _count(gpu, "sh1", k, dev, 0, 100, ptr)
    _, cnt = _table(ptr)
    assert cnt.max() >= 3 and len(cnt) > 1000 and len(set(cnt.tolist())) >= 2
    assert ((mc + 1) <= SPEC_LDS_BINS) == (mc <= 8191)
    got = api.kmer_spec_sh(ptr, mc)
    want = np.bincount(np.minimum(cnt, mc), minlength=mc + 1).astype(np.float64)
    assert got.shape == (mc + 1,) and np.array_equal(got, want)
    ptr.free()


@pytest.mark.parametrize("mc", (1364, 1365))
def test_spectrum_sh_n_lds_and_global_bins(gpu, mc, tmp_path):
    """kmer.spec.sh.n with S = 2 sources and 3 combinations: (max_count + 1) * 6 = 8,190 bins
    (LDS branch) and 8,196 (global atomics), against OracleSH.spectrum.  Two ragged files, the
    first counted into both sources."""
    from kmer_hasher_amd import api
    k, S = 21, 2
    fa = _ragged_file(tmp_path, k, 700, "a.fx")[0]
    fb = _ragged_file(tmp_path, k, 151, "b.fx")[0]
    ptr, o = None, O.OracleSH(k, S)
    for f, src in ((fa, 0), (fb, 1), (fa, 1)):
        ptr = api.count_kmers_fq_sh_rp(f, [k, 20, P.MQ_RP, 1, -1, 1, S, src], ptr)
        o.add_fastq(f, P.MQ_RP, 2**62, src)
    comb, inner, smin = [1, 2, 3], [1, 0, 1], [1, 2]
    assert (((mc + 1) * len(comb) * S) <= SPEC_LDS_BINS) == (mc == 1364)
    got = api.kmer_spec_sh_n(ptr, mc, comb, inner, smin)
    want = o.spectrum(mc, comb, inner, smin)
    assert want.sum() > 1000 and want[:, 2:].sum() > 0 and (want.sum(1) > 0).sum() >= 4
    assert got.shape == (len(comb) * S, mc + 1) and np.array_equal(got, want)
    ptr.free()


# ---------------------------------------------------------------- the host split
def _reads_of(path, k):
    from kmer_hasher_amd import _lib
    h = C.c_void_p()
    _lib.check(_lib.lib().kmhg_fastx_read(path.encode(), -1, k, C.byref(h)))
    return h


def _count_all_entries(path, k):
    """{entry: key-sorted table} of one file through the four host entries; every handle freed."""
    from kmer_hasher_amd import _lib, api
    L = _lib.lib()
    rp_prm, sh1_prm = [k, 10, P.MQ_RP, 1, -1, 1, 1, 0], I.params(k)
    out = {}
    for name, ptr in (("rp_file", api.count_kmers_fq_sh_rp(path, rp_prm)),
                      ("sh1_file", api.count_kmers_fq_sh(path, sh1_prm))):
        out[name] = _table(ptr)
        ptr.free()
    reads = _reads_of(path, k)
    try:
        for name, fn, prm, tag in (
                ("rp_reads", L.kmhg_sh_count_reads, (C.c_int32 * 8)(*rp_prm), api.SUFFIX_HASH_N_TAG),
                ("sh1_reads", L.kmhg_sh1_count_reads, (C.c_int32 * 6)(*sh1_prm),
                 api.SUFFIX_HASH_TAG)):
            h = C.c_void_p()
            _lib.check(fn(C.byref(h), reads, prm))
            ptr = api.ExtPtr(h.value, tag=tag)
            out[name] = _table(ptr)
            ptr.free()
    finally:
        L.kmhg_reads_free(reads)
    return out


def _ragged_file(tmp_path, k, max_len, name):
    # FASTA records first, as every mixed file the .rp reader is compared on (tests/sh_inputs.py)
    recs = P.ragged_records(P.SEEDS[k], k, 200, 1 / 3, max_len=max_len, nuls=False)
    recs = [r for r in recs if r[1] is None] + [r for r in recs if r[1] is not None]
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(I.fastx_bytes(recs))
    return p, recs


@pytest.mark.parametrize("k", (21,))
def test_host_split_by_span(gpu, test_lib, monkeypatch, tmp_path, k):
    """sh_count_reads_host's split (KMHG_SH_SPAN in the test build, 2^32 - 1 bases otherwise): one
    FASTX file and one kmhg_reads object of ~200 ragged records (longest 700) counted unsplit, in
    batches of < 4000 and of < 701 bases -- device calls at d_offsets + i0 with off[i0] != 0 --
    give one table, the oracle's, for both walks and both entries.  With 701, a record of 5000
    bases is refused (KMHG_EOVERFLOW) before anything is counted: the hash stays as it was."""
    from kmer_hasher_amd import _lib, api
    path, recs = _ragged_file(tmp_path, k, 700, "ragged.fx")
    kept = [r for r in recs if len(r[0]) > k]
    ln = np.array([len(r[0]) for r in kept])
    assert ln.max() == 700 and ln.sum() > 3 * 4000                # both spans really split
    assert (np.cumsum(ln)[:-1] % 16 != 0).any()
    want = {"rp": P.table_of_keys([P.rp_keys(r, k) for r in kept]),
            "sh1": P.table_of_keys([P.sh1_keys(r, k) for r in kept])}
    for span in (None, "4000", "701"):
        if span is None:
            monkeypatch.delenv("KMHG_SH_SPAN", raising=False)
        else:
            monkeypatch.setenv("KMHG_SH_SPAN", span)
        for name, (gk, gc) in _count_all_entries(path, k).items():
            wk, wc = want[name.split("_")[0]]
            assert len(wk) > 1000 and np.array_equal(gk, wk) and np.array_equal(gc, wc), \
                (span, name)
    # a record no batch can hold
    long_path, long_recs = _ragged_file(tmp_path, k, 5000, "long.fx")
    assert max(len(r[0]) for r in long_recs) == 5000
    monkeypatch.setenv("KMHG_SH_SPAN", "701")
    L = _lib.lib()
    rp_prm, sh1_prm = [k, 10, P.MQ_RP, 1, -1, 1, 1, 0], I.params(k)
    reads = _reads_of(long_path, k)
    try:
        for walk, count_file, fn, prm in (
                ("rp", api.count_kmers_fq_sh_rp, L.kmhg_sh_count_reads, rp_prm),
                ("sh1", api.count_kmers_fq_sh, L.kmhg_sh1_count_reads, sh1_prm)):
            ptr = count_file(path, prm)
            before = _table(ptr)
            with pytest.raises(_lib.KmhgError) as e:
                count_file(long_path, prm, ptr)
            assert e.value.code == _lib.KMHG_EOVERFLOW
            h = C.c_void_p(ptr.handle.value)
            assert fn(C.byref(h), reads, (C.c_int32 * len(prm))(*prm)) == _lib.KMHG_EOVERFLOW
            assert h.value == ptr.handle.value
            after = _table(ptr)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            assert np.array_equal(before[0], want[walk][0])
            fresh = C.c_void_p()
            assert fn(C.byref(fresh), reads, (C.c_int32 * len(prm))(*prm)) == _lib.KMHG_EOVERFLOW
            assert not fresh.value
            ptr.free()
    finally:
        L.kmhg_reads_free(reads)
