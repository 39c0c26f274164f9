"""count.kmers.fq.sh / kmer.spec.sh on the GPU against the compiled reference (tests/ref_fq_sh.py):
keys, counts and spectra compared exactly.  Lane-per-read walk (records with qualities) and
position-parallel kernel (records without) over the edge lists of tests/fq_sh_inputs.py, the
reference's own fixtures with test.R's parameter shapes, spectrum clamping, pointer kinds.

k = 31 needs a 30-bit prefix array in the reference, which its sh_count_spectrum walks in full
(seconds per call): there the spectra come from the golden file, which the same reference made
(tests/test_fq_sh_ref.py reproduces it)."""
import ctypes as C
import os

import numpy as np
import pytest

import fq_sh_inputs as I
import ref_fq_sh as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.available(), reason="oracle/_ref/libkmh_ref_sh.so not built")]
GOLD = {c["name"]: c for c in I.load_golden()["cases"]}


def _table(ptr):
    from kmer_hasher_amd import api
    keys, M = api.counts_table(ptr)
    o = np.argsort(keys, kind="stable")
    return keys[o], M[o, 0] if len(keys) else np.zeros(0, np.int32)


def _compare(ptr, ref, k, gold_name=None):
    from kmer_hasher_amd import api
    keys, cnt = _table(ptr)
    rk, rc = ref.arrays()
    assert np.array_equal(keys, rk) and np.array_equal(cnt, rc)
    inf = ptr.info()
    assert inf.kind == 3 and inf.sources == 1 and inf.k == k and inf.kmer_count == len(rk)
    for mc in I.SPECTRA:
        got = api.kmer_spec_sh(ptr, mc)
        if k < 31:
            want = ref.spectrum(mc)
        else:
            want = np.bincount(np.minimum(rc, mc), minlength=mc + 1).astype(np.float64)
            if gold_name:
                from kmh_canon import sha
                assert sha(got) == GOLD[gold_name]["spectra"][str(mc)]["sha"]
        assert got.dtype == np.float64 and np.array_equal(got, want), mc
    ref.close()


def _count_file(tmp_path, records, k, mq, name="in.fx"):
    from kmer_hasher_amd import api
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(I.fastx_bytes(records))
    return api.count_kmers_fq_sh(p, I.params(k, mq))


@pytest.mark.parametrize("k", I.LANE_KS)
def test_lane_per_read_edges(gpu, k, tmp_path):
    for name, (recs, mq) in I.lane_cases(k).items():
        ptr = _count_file(tmp_path, recs, k, mq)
        ref = R.RefSH1(k, I.prefix_bits_for(k)).add_records(recs, mq)
        assert len(ref.keys) == GOLD[f"lane_k{k}_{name}"]["U"]
        _compare(ptr, ref, k, f"lane_k{k}_{name}")
        ptr.free()


@pytest.mark.parametrize("k", I.FA_KS)
def test_position_parallel_edges(gpu, k, tmp_path):
    for name, recs in I.fa_cases(k).items():
        ptr = _count_file(tmp_path, recs, k, I.MQ)
        ref = R.RefSH1(k, I.prefix_bits_for(k)).add_records(recs, I.MQ)
        _compare(ptr, ref, k)
        ptr.free()


@pytest.mark.parametrize("name", list(I.FILE_CASES))
def test_reference_fixtures(gpu, name):
    """The reference's own files with test.R's parameter shapes; max_read_n 0 / 5 / -1; two calls
    accumulated into one pointer; test.fa as a FASTA input."""
    from kmer_hasher_amd import api
    calls = I.FILE_CASES[name]
    k = calls[0][1][0]
    ref = R.RefSH1(k, calls[0][1][2], calls[0][1][3])
    ptr = None
    for f, prm in calls:
        p = os.path.join(I.GOLDEN, f)
        nxt = api.count_kmers_fq_sh(p, prm, ptr)
        assert ptr is None or nxt is ptr
        ptr = nxt
        ref.add_fastx(p, prm)
    assert ptr.tag == api.SUFFIX_HASH_TAG
    _compare(ptr, ref, k, name)


def test_device_entry_routes_by_record(gpu):
    """kmhg_sh1_count_reads_device on packed reads, every third one without qualities (so both
    kernels write into one key stream), one with a NUL inside: against the reference."""
    torch = gpu
    from kmer_hasher_amd import _lib, api
    k, n, rl = 21, 200, 150
    rng = np.random.default_rng(5)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, rl))
    seq[rng.random((n, rl)) < 0.01] = ord("N")
    seq[7, 90] = 0
    seq[9, 100] = 0                                   # in a record without qualities
    qual = rng.choice(np.array([I.GOOD, I.WEAK, I.BAD], np.uint8), (n, rl), p=[.9, .06, .04])
    hasq = (np.arange(n) % 3 != 0).astype(np.uint8)
    flat = np.zeros(n * rl + 16, np.uint8)
    flat[:n * rl] = seq.reshape(-1)
    qf = np.zeros(n * rl + 16, np.uint8)
    qf[:n * rl] = qual.reshape(-1)
    off = np.arange(n + 1, dtype=np.int64) * rl
    t = [torch.from_numpy(a).to("cuda") for a in (flat, qf, off, hasq)]
    h = C.c_void_p()
    prm = (C.c_int32 * 6)(*I.params(k))
    _lib.check(_lib.lib().kmhg_sh1_count_reads_device(C.byref(h), t[0].data_ptr(), t[1].data_ptr(),
                                                      t[2].data_ptr(), t[3].data_ptr(), n, prm,
                                                      None))
    torch.cuda.synchronize()
    ptr = api.ExtPtr(h.value, tag=api.SUFFIX_HASH_TAG)
    recs = [(s.tobytes(), q.tobytes() if hq else None) for s, q, hq in zip(seq, qual, hasq)]
    _compare(ptr, R.RefSH1(k, I.prefix_bits_for(k)).add_records(recs, I.MQ), k)


def test_spectrum_clamp(gpu):
    """max_count = 1, below the largest count (the clamp bin) and above it."""
    from kmer_hasher_amd import api
    p = os.path.join(I.GOLDEN, "repeat_40.fq")
    prm = [20, 1, 20, 100, 0, -1]
    ptr = api.count_kmers_fq_sh(p, prm)
    ref = R.RefSH1(20, 20).add_fastx(p, prm)
    top = int(ref.arrays()[1].max())
    assert top > 3
    for mc in (1, top - 1, top + 5):
        got = api.kmer_spec_sh(ptr, mc)
        assert got.shape == (mc + 1,) and got[0] == 0
        assert np.array_equal(got, ref.spectrum(mc)), mc
    assert api.kmer_spec_sh(ptr, top - 1)[top - 1] >= 1          # the clamp bin holds the top
    for bad in (0, -1, (1 << 30) + 1):
        with pytest.raises(api.KmerHashError, match="^Unsuitable value of max_count$"):
            api.kmer_spec_sh(ptr, bad)


def test_pointer_kinds(gpu):
    from kmer_hasher_amd import _lib, api
    E = api.KmerHashError
    L = _lib.lib()
    p = os.path.join(I.GOLDEN, "test_10.fastq")
    one = api.count_kmers_fq_sh(p, [20, 1, 20, 100, 30, -1])
    rp = api.count_kmers_fq_sh_rp(p, [20, 20, 30, 1, -1, 1, 1, 0])
    assert one.info().kind == 3 and rp.info().kind == 2
    # the suffix_hash_n readers refuse a single suffix hash: front end (tag) and C-ABI (kind)
    with pytest.raises(E, match="unable to obtain suffix_hash_n from external pointer"):
        api.seq_kmer_depth_sh(one, "ACGT" * 10, 20)
    with pytest.raises(E, match="unable to obtain suffix_hash_n from external pointer"):
        api.kmer_spec_sh_n(one, 5, [1], [0], [1])
    out = np.zeros(64, np.int32)
    assert L.kmhg_sh_depth(one.handle, b"ACGT" * 10, 40, 20, out.ctypes.data) == _lib.KMHG_EINVAL
    assert b"suffix_hash_n" in L.kmhg_last_error()
    st = C.c_int()
    a1 = np.array([1], np.int32)
    d = np.zeros(8, np.float64)
    assert L.kmhg_sh_spectrum(one.handle, 5, a1.ctypes.data, a1.ctypes.data, 1, a1.ctypes.data, 1,
                              d.ctypes.data, C.byref(st)) == _lib.KMHG_EINVAL
    # and the single-hash entries refuse a suffix_hash_n
    with pytest.raises(E, match="^unable to obtain a suffix_hash from external pointer$"):
        api.kmer_spec_sh(rp, 5)
    assert L.kmhg_sh1_spectrum(rp.handle, 5, d.ctypes.data) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "unable to obtain a suffix_hash from external pointer"
    h = C.c_void_p(rp.handle.value)
    prm = (C.c_int32 * 6)(20, 1, 20, 100, 30, -1)
    assert L.kmhg_sh1_count_fastq(C.byref(h), p.encode(), prm) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "Unable to extract suffix_hash from external pointer"
    with pytest.raises(E, match="^Unable to extract suffix_hash from external pointer$"):
        api.count_kmers_fq_sh(p, [20, 1, 20, 100, 30, -1], rp)
    # a different k into an existing single suffix hash is refused, and nothing changes
    before = _table(one)
    with pytest.raises(E, match="^k differs from the k of the suffix hash$"):
        api.count_kmers_fq_sh(p, [21, 1, 20, 100, 30, -1], one)
    after = _table(one)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    with pytest.raises(E, match="incorrect tag"):
        api.kmer_pos(one, 15)
