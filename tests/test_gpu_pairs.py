"""kmer.pairs (kmer_pair_pos, reference src/kmer_hash.c:1174-1203) on the GPU against the oracle.

The reference implementation crashes (test.R:330), so no reference output exists to pin this
row: parity is against the oracle's restatement of the intended loop (OracleIndex.pairs_with),
the checker being pinned on the rest of the index by test_oracle_golden.py."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _mutate(s: bytes, rate: float, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    a = np.frombuffer(s, np.uint8).copy()
    hit = rng.random(len(a)) < rate
    a[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, hit.sum())]
    return a.tobytes()


def test_pairs_match_oracle(gpu):
    from kmer_hasher_amd import kmer_pairs, make_kmer_hash, set_row_order, synth
    a = synth.add_n_runs(synth.repeat_rich(80_000, 9, n_gap_every=30_000), 0.002, 4).tobytes()
    b = _mutate(a[20_000:] + a[:20_000], 0.01, 2)
    for k in (11, 21, 31, 32):
        pa, pb = make_kmer_hash(a.decode("latin-1"), k), make_kmer_hash(b.decode("latin-1"), k)
        oa, ob = O.OracleIndex(a, k), O.OracleIndex(b, k)
        got = kmer_pairs(pa, pb)
        want = oa.pairs_with(ob)
        assert got.shape[1] == 2 and len(want) > 0
        assert np.array_equal(got.reshape(-1), want), k
        # b against a, and a against itself
        assert np.array_equal(kmer_pairs(pb, pa).reshape(-1), ob.pairs_with(oa)), k
        assert np.array_equal(kmer_pairs(pa, pa).reshape(-1), oa.pairs_with(oa)), k
        # a's k-mers in the reference's khash order, as the reference's bucket walk visits them
        set_row_order(pa, "khash")
        assert np.array_equal(kmer_pairs(pa, pb).reshape(-1), oa.pairs_with(ob, oa.khash_order()))
        pa.free()
        pb.free()


def test_pairs_edge_cases(gpu):
    from kmer_hasher_amd import KmerHashError, kmer_pairs, make_kmer_hash
    p1 = make_kmer_hash("AAAAAAAAAA", 3)
    p2 = make_kmer_hash("CCCCCCCCCC", 3)
    assert kmer_pairs(p1, p2).shape == (0, 2)             # nothing shared
    p3 = make_kmer_hash("AAAAAAAAAAAAAAAA", 3)            # one k-mer, many positions
    got = kmer_pairs(p1, p3)
    want = O.OracleIndex("AAAAAAAAAA", 3).pairs_with(O.OracleIndex("AAAAAAAAAAAAAAAA", 3))
    assert np.array_equal(got.reshape(-1), want)
    p4 = make_kmer_hash("AAAAAAAAAA", 4)
    with pytest.raises(KmerHashError, match="the two indices must have the same k"):
        kmer_pairs(p1, p4)
    g = make_kmer_hash("G" * 40, 32)                      # the k = 32 side-slot key
    assert np.array_equal(kmer_pairs(g, g).reshape(-1),
                          O.OracleIndex("G" * 40, 32).pairs_with(O.OracleIndex("G" * 40, 32)))


# ------------------------------------------------------------------------------------------
# The named inputs of pairs_inputs.py (tile edges, heavy keys, inline / listed positions, table
# geometries, the side slot, counts indices) against pairs_ref, the plain-Python restatement;
# test_pairs_ref.py holds pairs_ref to OracleIndex.pairs_with on the same inputs and shows that
# each input changes under the kernel defect it was built for.  Every comparison is exact.
import ctypes as C  # noqa: E402
import time  # noqa: E402

import pairs_inputs as I  # noqa: E402
import pairs_ref as R  # noqa: E402
import raster_ref  # noqa: E402

PART_WORDS = "a part index must be assembled before it is read"


def _pair(name, d):
    from kmer_hasher_amd import make_kmer_hash
    x, y = I.sides(name, d)
    k = I.case(name).k
    px = make_kmer_hash(x, k)
    return px, (px if d == "aa" else make_kmer_hash(y, k))


@pytest.mark.parametrize("name,d", I.RUNS)
def test_named_cases_match_pairs_ref(gpu, name, d):
    from kmer_hasher_amd import kmer_pairs
    px, py = _pair(name, d)
    got = kmer_pairs(px, py)
    assert got.dtype == np.int32 and got.shape == (len(I.want(name, d)) // 2, 2)
    assert np.array_equal(got.reshape(-1), I.want(name, d))
    px.free()
    py.free()


def test_a_string_of_length_k_is_not_built(gpu):
    from kmer_hasher_amd import KmerHashError, make_kmer_hash
    s, k = I.SHORT_A
    with pytest.raises(KmerHashError, match="the length of the sequence must be at least k"):
        make_kmer_hash(s, k)


@pytest.mark.parametrize("name", ["heavy_rank_2047", "holes", "n_and_case", "side_both", "ua_6151"])
def test_self_pairs_are_the_squares_of_kmer_pos(gpu, name):
    """a against itself from kmer.pos alone: every key gives count^2 rows, the cross product of its
    ascending positions with themselves, keys in kmer.pos row order."""
    from kmer_hasher_amd import kmer_pairs, kmer_pos, make_kmer_hash
    c = I.case(name)
    pa = make_kmer_hash(c.a, c.k)
    res = kmer_pos(pa, 2 | 8)
    cnt, pos = res["count"].astype(np.int64), res["pos"][:, 1]
    off = np.concatenate([[0], np.cumsum(cnt)])
    lists = [pos[off[i]:off[i + 1]] for i in range(len(cnt))]
    want = np.concatenate([np.stack([np.repeat(p, len(p)), np.tile(p, len(p))], 1) for p in lists])
    got = kmer_pairs(pa, pa)
    assert len(got) == int((cnt * cnt).sum())
    assert np.array_equal(got, want.astype(np.int32))
    pa.free()


@pytest.mark.parametrize("v1_side", ["a", "b"])
@pytest.mark.parametrize("d", ["ab", "ba"])
def test_geometry_with_one_side_from_the_fallback_build(gpu, test_lib, monkeypatch, d, v1_side):
    """200 characters against 400,000 and the reverse, one side a single bucket of global linear
    probing (KMHG_BUILD=v1), the other the partitioned table."""
    from kmer_hasher_amd import _lib, kmer_pairs, make_kmer_hash
    x, y = I.sides("geometry", d)
    k = I.case("geometry").k

    def make(s, v1):
        if v1:
            monkeypatch.setenv("KMHG_BUILD", "v1")
        else:
            monkeypatch.delenv("KMHG_BUILD", raising=False)
        p = make_kmer_hash(s, k)
        assert (p.info().build == _lib.KMHG_BUILD_GLOBAL) == v1
        return p

    px, py = make(x, v1_side == "a"), make(y, v1_side == "b")
    assert np.array_equal(kmer_pairs(px, py).reshape(-1), I.want("geometry", d))
    px.free()
    py.free()


def _table(name):
    from kmer_hasher_amd import count_kmers, make_kmer_hash
    k, S, x = I.count_specs()[name]
    if S == 0:
        return make_kmer_hash(x, k)
    ptr = None
    for source, seqs in x:
        ptr = count_kmers(list(seqs), (k, source, S), ptr)
    return ptr


@pytest.mark.parametrize("na,nb", I.COUNT_RUNS)
def test_counts_indices_pair_by_their_count_vectors(gpu, na, nb):
    """A counts index keeps the position index's slot convention (count = source_n, aux inline
    for source_n = 1, else the end of the row's vector), so kmer.pairs reads its count vectors
    where a position index has positions: counts x counts, position x counts, counts x position,
    source_n 1 and 3, one batch (the adopted table) and several (the rebuilt one, known keys
    re-counted).  The table is current after the last batch with no further step."""
    from kmer_hasher_amd import kmer_pairs
    pa = _table(na)
    pb = pa if na == nb else _table(nb)
    assert pa.info().sources == I.count_specs()[na][1]
    assert np.array_equal(kmer_pairs(pa, pb).reshape(-1), I.count_want(na, nb))
    pa.free()
    pb.free()


@pytest.mark.parametrize("table", ["adopt", "rebuild", "probe"])
def test_counts_indices_pair_on_every_counts_table(gpu, test_lib, monkeypatch, table):
    """... whichever way the counts table was made (KMHG_COUNT_TABLE: the first batch's table
    adopted, the partitioned build over the key list, one bucket of global linear probing)."""
    from kmer_hasher_amd import kmer_pairs
    monkeypatch.setenv("KMHG_COUNT_TABLE", table)
    for na, nb in (("c1_multi", "c3_multi"), ("pos1", "c3_single"), ("c1_single", "pos2")):
        pa, pb = _table(na), _table(nb)
        assert np.array_equal(kmer_pairs(pa, pb).reshape(-1), I.count_want(na, nb)), (na, nb)
        pa.free()
        pb.free()


def test_khash_row_order_and_back(gpu):
    from kmer_hasher_amd import kmer_pairs, set_row_order
    c = I.case("khash")
    pa, pb = _pair("khash", "ab")
    first = kmer_pairs(pa, pb)
    assert np.array_equal(first.reshape(-1), I.want("khash", "ab"))
    set_row_order(pa, "khash")
    order = O.OracleIndex(c.a, c.k).khash_order()
    assert np.array_equal(kmer_pairs(pa, pb).reshape(-1), R.pairs_ref(c.a, c.b, c.k, order))
    set_row_order(pa, "first")
    assert kmer_pairs(pa, pb).tobytes() == first.tobytes()
    pa.free()
    pb.free()


@pytest.mark.parametrize("name", ["holes", "heavy_rank_2047"])
def test_two_calls_give_identical_bytes(gpu, name):
    from kmer_hasher_amd import kmer_pairs
    px, py = _pair(name, "ab")
    one, two = kmer_pairs(px, py), kmer_pairs(px, py)
    assert one.tobytes() == two.tobytes() == I.want(name, "ab").tobytes()
    px.free()
    py.free()


def _tensor(torch, s: bytes):
    return torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()


def _run(L, a, b, entry="kmhg_pairs_run", stream=None, with_q=True):
    """(return code, query handle, n_rows) of one call through the C entry."""
    q, h = C.c_void_p(), C.c_int64(-1)
    args = [a, b] + ([stream] if entry.endswith("_device") else [])
    rc = getattr(L, entry)(*args, C.byref(q) if with_q else None, C.byref(h))
    return rc, q, h.value


def _host_rows(L, a, b) -> np.ndarray:
    from kmer_hasher_amd import _lib
    rc, q, h = _run(L, a, b)
    _lib.check(rc)
    rows = np.empty(2 * h, np.int32)
    if h:
        _lib.check(L.kmhg_query_fill(q, rows.ctypes.data))
    L.kmhg_query_free(q)
    return rows


@pytest.mark.parametrize("name", ["heavy_rank_2047", "holes"])
def test_pairs_run_device_on_the_callers_stream(gpu, name):
    """kmhg_pairs_run_device on a side stream: the library leaves the emit queued, the caller
    synchronises and reads the handle's device rows; byte for byte the rows of kmhg_pairs_run on
    the same handles, also after a query of b has run on a third stream in between."""
    torch = gpu
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex, DeviceQuery
    L = _lib.lib()
    c = I.case(name)
    ta, tb = _tensor(torch, c.a), _tensor(torch, c.b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ia, ib = DeviceIndex.build(ta, c.k, stream=s1), DeviceIndex.build(tb, c.k, stream=s1)

    def on_s1() -> bytes:
        rc, q, h = _run(L, ia.handle, ib.handle, "kmhg_pairs_run_device", C.c_void_p(s1.cuda_stream))
        _lib.check(rc)
        s1.synchronize()                                  # the entry does not
        rows = DeviceQuery(q.value, h, ta.device).rows_view()
        assert rows.shape == (h, 2) and rows.device == ta.device
        return rows.cpu().numpy().tobytes()

    want = I.want(name, "ab").tobytes()
    assert on_s1() == want
    assert _host_rows(L, ia.handle, ib.handle).tobytes() == want
    qb = ib.query(tb, c.k, stream=s2)
    s2.synchronize()
    assert qb.n_rows >= len(c.b) - c.k                    # (every window of b finds itself)
    qb.free()
    assert on_s1() == want
    ia.free()
    ib.free()


@pytest.mark.parametrize("name", ["holes", "n_and_case"])
def test_rows_raster_bins_pairs_rows(gpu, name):
    torch = gpu
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex, DeviceQuery, rows_raster
    L = _lib.lib()
    c = I.case(name)
    ta, tb = _tensor(torch, c.a), _tensor(torch, c.b)
    ia, ib = DeviceIndex.build(ta, c.k), DeviceIndex.build(tb, c.k)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc, q, h = _run(L, ia.handle, ib.handle, "kmhg_pairs_run_device", s)
    _lib.check(rc)
    rows = DeviceQuery(q.value, h, ta.device).rows_view()
    frame = (1, 1, -(-len(c.a) // 64), -(-len(c.b) // 64), 64, 64)
    got = rows_raster(rows, frame).cpu().numpy()
    want = raster_ref.raster(I.want(name, "ab"), frame)
    assert int(want.sum()) == h == len(I.want(name, "ab")) // 2     # the frame holds every row
    assert np.array_equal(got, want)
    del rows
    ia.free()
    ib.free()


def test_refusals_in_their_words(gpu):
    """Each refusal of kmhg_pairs_run[_device], in its words, and after each a normal call on the
    same library gives the right rows.  A part is refused as a and as b: the probe would hash
    over the part's own bucket count and report misses."""
    torch = gpu
    from kmer_hasher_amd import KmerHashError, _lib, api, kmer_pairs
    from kmer_hasher_amd.device import DeviceIndex
    L = _lib.lib()
    c = I.case("heavy_rank_0")
    ta, tb = _tensor(torch, c.a), _tensor(torch, c.b)
    ia, ib = DeviceIndex.build(ta, c.k), DeviceIndex.build(tb, c.k)
    want = I.want("heavy_rank_0", "ab")

    def refused(a, b, words, with_q=True):
        for entry in ("kmhg_pairs_run", "kmhg_pairs_run_device"):
            rc, q, _ = _run(L, a, b, entry, None, with_q)
            assert rc == _lib.KMHG_EINVAL and not q.value, (entry, words)
            assert L.kmhg_last_error().decode() == words, entry
        assert np.array_equal(_host_rows(L, ia.handle, ib.handle), want), words   # and it goes on

    for p, n in ((0, 2), (1, 2), (2, 3)):
        part = DeviceIndex.build_part(ta, c.k, p, n)
        refused(part.handle, ib.handle, PART_WORDS)
        refused(ia.handle, part.handle, PART_WORDS)
        refused(part.handle, part.handle, PART_WORDS)
        part.free()
    other_k = DeviceIndex.build(ta, c.k - 1)
    refused(ia.handle, other_k.handle, "the two indices must have the same k")
    refused(other_k.handle, ib.handle, "the two indices must have the same k")
    sh = api.count_kmers_fq_sh_rp("no-such-file.fq", [15, 10, 0, 1, -1, 1, 1, 0])
    refused(sh.handle, ib.handle, "External pointer has incorrect tag")
    refused(ia.handle, sh.handle, "External pointer has incorrect tag")
    pa = api.make_kmer_hash(c.a, c.k)
    for x, y in ((sh, pa), (pa, sh)):
        with pytest.raises(KmerHashError, match="^External pointer has incorrect tag$"):
            kmer_pairs(x, y)
    refused(None, ib.handle, "null argument")
    refused(ia.handle, None, "null argument")
    refused(ia.handle, ib.handle, "null argument", with_q=False)
    for x in (other_k, ia, ib, sh, pa):
        x.free()


def test_two_devices_are_refused(gpu):
    torch = gpu
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex
    L = _lib.lib()
    c = I.case("heavy_rank_0")
    ta, tb = _tensor(torch, c.a), _tensor(torch, c.b)
    ia, ib = DeviceIndex.build(ta, c.k), DeviceIndex.build(tb, c.k)
    far = DeviceIndex.build(tb.to("cuda:1"), c.k)
    for x, y in ((ia, far), (far, ia)):
        rc, q, _ = _run(L, x.handle, y.handle)
        assert rc == _lib.KMHG_EINVAL and not q.value
        assert L.kmhg_last_error().decode() == "the two indices must be on the same device"
    assert np.array_equal(_host_rows(L, ia.handle, ib.handle), I.want("heavy_rank_0", "ab"))
    for x in (ia, ib, far):
        x.free()


@pytest.mark.slow
def test_rows_past_2_31(gpu):
    """46,341 x A against itself at k = 1: one key, one tile, 46,341^2 = 2,147,488,281 rows, so
    row offsets pass 2^31 inside one workgroup's loop.  The device entry holds them all (17 GB):
    row r is (r // n + 1, r % n + 1).  kmer.pairs refuses the host matrix, as seq.kmer.pos does
    (test_query_rows_over_int_max_raise).  One workgroup deals all of these rows, twice (the
    device entry, then kmer.pairs before it refuses): more than 5 s, hence `slow`."""
    torch = gpu
    from kmer_hasher_amd import KmerHashError, _lib, kmer_pairs, make_kmer_hash
    from kmer_hasher_amd.device import DeviceQuery
    L = _lib.lib()
    n = 46_341
    t0 = time.perf_counter()
    ptr = make_kmer_hash("A" * n, 1)
    assert (ptr.info().n_kmers, ptr.info().n_positions) == (1, n)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc, q, h = _run(L, ptr.handle, ptr.handle, "kmhg_pairs_run_device", s)
    _lib.check(rc)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    assert h == n * n == 2_147_488_281 > 2**31
    rows = DeviceQuery(q.value, h, torch.device("cuda", torch.cuda.current_device())).rows_view()
    assert rows.shape == (h, 2)
    for lo, hi in ((0, 8192), (2**31 - 8192, 2**31 + 4096), (h - 8192, h)):
        r = np.arange(lo, hi, dtype=np.int64)
        want = np.stack([r // n + 1, r % n + 1], 1).astype(np.int32)
        assert np.array_equal(rows[lo:hi].cpu().numpy(), want), lo
    del rows
    with pytest.raises(KmerHashError, match="2\\^31-1 columns"):
        kmer_pairs(ptr, ptr)
    ptr.free()
    L.kmhg_pool_trim()
    t2 = time.perf_counter()
    print(f"rows past 2^31: device entry {t1 - t0:.2f} s, whole test {t2 - t0:.2f} s")
