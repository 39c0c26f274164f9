"""(w,k)-minimizer sampling on the GPU (kmhg_build_sampled*, kmhg_minimizer_mask_device;
kmhg_minimizer.hip): the selection kernel against the host function of the shared header, and a
sampled index in every product against tests/minimizer_ref.py -- the oracle's k-mers, positions and
rows restricted to the reference masks -- fed to segs_ref / blocks_ref / chains_ref / raster_ref.
Integer work: every comparison is exact, order included.  The selection kernel walks tiles of
2,048 windows with a halo of w - 1 windows on both sides, so the shapes sit around one and two
tiles and put minima, spans and Ns across tile edges."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import blocks_ref
import chains_ref
import minimizer_ref
import pairs_ref
import raster_ref
import segs_ref

pytestmark = pytest.mark.gpu

TILE = 2048


def _iid(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


def _seq_t(torch, s):
    a = np.frombuffer(s.encode("latin-1"), np.uint8) if isinstance(s, str) else s
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _rows(q):
    r = q.rows().cpu().numpy()
    q.free()
    return r


def _device_mask(torch, s, k, w, rc):
    """The kernel's mask as one byte per window, and its count."""
    from kmer_hasher_amd.device import DeviceIndex
    words, n = DeviceIndex.minimizer_mask(_seq_t(torch, s), k, w, rc)
    nw = len(s) - k + 1
    assert words.numel() == (nw + 31) // 32
    bits = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")
    assert not bits[nw:].any()                       # bits past Nw are zero
    return bits[:nw], n


def _host_mask(s, k, w, rc):
    from kmer_hasher_amd import minimizer_mask
    return minimizer_mask(s, k, w, rc)


def _check_mask(torch, s, k, w):
    for rc in (False, True):
        got, n = _device_mask(torch, s, k, w, rc)
        want = _host_mask(s, k, w, rc)
        assert np.array_equal(got, want), (len(s), k, w, rc, np.flatnonzero(got != want)[:8])
        assert n == int(want.sum())


# ------------------------------------------------------------------ 1. the selection kernel
@pytest.mark.parametrize("k", [5, 15, 31])
def test_mask_kernel_tile_shapes(gpu, k):
    """Nw one below, at and one above a tile, and two tiles plus 1."""
    s = _iid(2 * TILE + 1 + k - 1, 11 + k)
    for nw in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        for w in (1, 2, 10, 64, 256):
            _check_mask(gpu, s[:nw + k - 1], k, w)


def test_mask_kernel_w_near_the_window_count(gpu):
    s = _iid(400, 3)
    for k in (5, 31):
        for w in (1, 2, 64, 255, 256):
            for nw in (w - 1, w, w + 1, w + 2):
                if nw >= 2:
                    _check_mask(gpu, s[:nw + k - 1], k, w)


def test_mask_kernel_minima_and_ns_at_tile_edges(gpu):
    """A minimum in the last window of tile 0, every span of which but one reaches into tile 1,
    the mirror case (the first window of tile 1, spans beginning in tile 0), and an N exactly w
    windows after the edge, which cuts the spans that cross it."""
    k, w = 15, 64
    base = _iid(2 * TILE + 500, 77)
    h = minimizer_ref.hashes(base, k)
    # a window that is the strict minimum of all 2 w - 1 windows around it: selected by every span
    p = next(p for p in range(TILE + w, 2 * TILE)
             if h[p] == h[p - w + 1:p + w].min() and (h[p - w + 1:p + w] == h[p]).sum() == 1)
    for target in (TILE - 1, TILE):                  # the 0-based window it is moved to
        s = base[p - target:]
        m = _host_mask(s, k, w, False)
        assert m[target] == 1 and len(s) - k + 1 > TILE + w
        _check_mask(gpu, s, k, w)
    for k2, w2 in ((15, 64), (5, 255), (31, 2)):
        s = list(base)
        s[TILE + w2] = "N"                           # the char at window start TILE + w2
        _check_mask(gpu, "".join(s), k2, w2)
        s[TILE + w2 + k2 - 1] = "n"
        s[5] = "N"
        s[-k2 - 1] = "N"                             # before the last window: the end-drop rule
        _check_mask(gpu, "".join(s), k2, w2)


def test_mask_kernel_equal_hashes_break_ties_to_the_left(gpu):
    for w in (2, 19, 256):
        _check_mask(gpu, "A" * 70000, 15, w)
        _check_mask(gpu, "ACG" * 2000, 5, w)
    got, n = _device_mask(gpu, "A" * 70000, 31, 10, False)
    nw = 70000 - 31 + 1
    assert np.array_equal(got, (np.arange(nw) + 10 <= nw).astype(np.uint8)) and n == nw - 9


# ------------------------------------------------------------------ 2. w = 1 is today's build
def test_w1_through_the_new_entry_is_the_old_index(gpu, testfa):
    torch = gpu
    from kmer_hasher_amd import get_sampling, kmer_pos, make_kmer_hash, seq_kmer_pos, set_row_order
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex
    s = testfa[:6000]
    k = 15
    t = _seq_t(torch, s)
    old = DeviceIndex.build(t, k)
    new = C.c_void_p()
    _lib.check(_lib.lib().kmhg_build_sampled_device(C.c_void_p(t.data_ptr()), t.numel(), k, 1, 0,
                                                    None, C.byref(new)))
    torch.cuda.synchronize()
    new = DeviceIndex(new.value)
    assert old.sampling == 1 and new.sampling == 1
    for opt in (1, 2, 4, 8, 15):
        a, b = old.positions(opt), new.positions(opt)
        for f in a:
            assert (a[f] is None) == (b[f] is None)
            if a[f] is not None:
                assert torch.equal(a[f], b[f]), (opt, f)
    assert np.array_equal(_rows(old.query(t, k)), _rows(new.query(t, k)))
    old.free()
    new.free()
    # the host entries: make_kmer_hash(w=1) is make_kmer_hash, both row orders
    p0, p1 = make_kmer_hash(s, k), make_kmer_hash(s, k, False, 1)
    assert get_sampling(p0) == 1 and get_sampling(p1) == 1
    for order in ("first", "khash"):
        set_row_order(p0, order)
        set_row_order(p1, order)
        a, b = kmer_pos(p0, 15), kmer_pos(p1, 15)
        assert a["kmer"] == b["kmer"]
        for f in ("pos", "pair.pos", "count"):
            assert np.array_equal(a[f], b[f]), (order, f)
    assert np.array_equal(seq_kmer_pos(p0, s, k), seq_kmer_pos(p1, s, k))
    p0.free()
    p1.free()


# ------------------------------------------------------------------ 3. sampled indexes
def _mutated(s, seed):
    """1 % substitutions and a few indels."""
    rng = np.random.default_rng(seed)
    a = list(s)
    for p in rng.choice(len(a), len(a) // 100, replace=False):
        a[p] = "ACGT"[("ACGT".find(a[p].upper()) + 1 + int(rng.integers(3))) % 4]
    for p in sorted(rng.choice(len(a) - 10, 6, replace=False).tolist(), reverse=True):
        if p % 2:
            del a[p:p + 1 + p % 3]
        else:
            a[p:p] = list(_iid(1 + p % 4, p))
    return "".join(a)


@pytest.fixture(scope="module")
def inputs(testfa):
    fa = testfa[:6000]
    rnd = list(_iid(50_000, 99))
    rnd[20_000:20_037] = "N" * 37
    rnd = "".join(rnd)
    return {"fa": (fa, 15), "rnd": (rnd, 15)}


@pytest.fixture(scope="module")
def oracles(inputs):
    """Per input: the oracle's index and its unsampled rows for the three queries, once."""
    out = {}
    for name, (s, k) in inputs.items():
        ox = O.OracleIndex(s, k)
        qs = {"self": s, "mutated": _mutated(s, 5), "unrelated": _iid(len(s) // 2, 1234)}
        rows = {}
        for qn, q in qs.items():
            rows[qn, False] = ox.query(q, k).reshape(-1, 2)
            rows[qn, True] = ox.query(rc_host(q), k).reshape(-1, 2)
        out[name] = ox, qs, rows
    return out


def _first_order(keys, positions_of):
    """keys ordered by their first position."""
    return sorted(keys, key=lambda x: positions_of[x][0])


@pytest.mark.parametrize("w", [2, 5, 19])
@pytest.mark.parametrize("name", ["fa", "rnd"])
def test_sampled_kmer_pos(gpu, inputs, oracles, name, w):
    """kmer.pos of the sampled index: the oracle's k-mers and positions restricted to the
    reference mask, labelled by first surviving occurrence, and in khash order by the library's
    kmhg_khash_order replayed on the surviving keys in that order."""
    from kmer_hasher_amd import _lib, get_sampling, kmer_pos, make_kmer_hash, set_row_order
    s, k = inputs[name]
    ox = oracles[name][0]
    imask = minimizer_ref.mask(s, k, w)
    pos_of = {}
    for u in range(ox.U):
        p = ox.positions[ox.offsets[u]:ox.offsets[u + 1]]
        p = p[imask[p.astype(np.int64) - 1] != 0]
        if len(p):
            pos_of[int(ox.keys[u])] = np.sort(p)
    keys = _first_order(list(pos_of), pos_of)
    assert 0 < len(keys) < ox.U
    ptr = make_kmer_hash(s, k, False, w)
    assert get_sampling(ptr) == w
    inf = ptr.info()
    assert inf.n_kmers == len(keys) and inf.n_positions == int(imask.sum())
    order = np.empty(len(keys), np.uint32)
    _lib.check(_lib.lib().kmhg_khash_order(
        np.array(keys, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), len(keys),
        order.ctypes.data_as(C.POINTER(C.c_uint32))))
    for mode, ids in (("first", list(range(len(keys)))), ("khash", order.tolist())):
        set_row_order(ptr, mode)
        got = kmer_pos(ptr, 15)
        lab = [keys[i] for i in ids]
        assert got["kmer"] == [O.decode(x, k) for x in lab], mode
        cnt = np.array([len(pos_of[x]) for x in lab], np.int32)
        assert np.array_equal(got["count"], cnt), mode
        want = np.stack([np.repeat(np.arange(1, len(lab) + 1, dtype=np.int32), cnt),
                         np.concatenate([pos_of[x] for x in lab]).astype(np.int32)], 1)
        assert np.array_equal(got["pos"], want), mode
        assert len(got["pair.pos"]) == int((cnt.astype(np.int64) * (cnt - 1) // 2).sum()), mode
    ptr.free()


def _check_products(torch, idx, t, k, rc, want, frames):
    dq = idx.query_rc(t, k) if rc else idx.query(t, k)
    assert dq.n_rows == len(want)
    assert np.array_equal(dq.rows().cpu().numpy(), want)
    segs = segs_ref.segments(want)
    for ml in (1, 2):
        got, h = idx.segments(t, k, ml, rc=rc)
        ws = segs[segs[:, 2] >= ml]
        assert h == len(want) and got.shape == ws.shape and np.array_equal(got.cpu().numpy(), ws)
        assert torch.equal(got, dq.segments(ml)), ("segments: the two routes", ml)
    for gap, ml, mh in ((k, 1, 1), (40, 1, 2)):
        got, h = idx.blocks(t, k, gap, ml, mh, rc=rc)
        wb = blocks_ref.merge(segs[segs[:, 2] >= ml], gap, mh)
        assert h == len(want) and got.shape == wb.shape and np.array_equal(got.cpu().numpy(), wb)
        assert torch.equal(got, dq.blocks(gap, ml, mh)), ("blocks: the two routes", gap, ml, mh)
    wb = blocks_ref.merge(segs, 40, 1)
    wc, wm = chains_ref.chains(wb, 5000, 500, 1)
    for rf in (False, True):
        c, b, m, h = idx.chains(t, k, 5000, 500, 40, 1, 1, rc=rc, row_free=rf)
        assert h == len(want), (rf, h)
        assert b.shape == wb.shape and np.array_equal(b.cpu().numpy(), wb), rf
        assert c.shape == wc.shape and np.array_equal(c.cpu().numpy(), wc), rf
        assert np.array_equal(m.cpu().numpy(), wm), rf
    from kmer_hasher_amd.device import rows_raster
    for f in frames:
        got, h = idx.raster(t, k, f, rc=rc)
        assert h == len(want)
        assert np.array_equal(got.cpu().numpy(), raster_ref.raster(want, f)), f
        assert torch.equal(got, dq.raster(f)), ("raster: the two routes", f)
        if len(want):
            assert torch.equal(got, rows_raster(dq.rows(), f)), ("rows_raster", f)
    dq.free()


def _sampled_occurrences(ox, imask):
    """occ[j] = at how many SELECTED positions the k-mer indexed at position j (1-based) occurs:
    the count kmer.max.occ sees, since the sampled index holds the selected positions alone."""
    occ = np.zeros(len(imask) + 2, np.int64)
    for u in range(ox.U):
        p = ox.positions[ox.offsets[u]:ox.offsets[u + 1]].astype(np.int64)
        p = p[imask[p - 1] != 0]
        occ[p] = len(p)
    return occ


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("w", [2, 5, 19])
@pytest.mark.parametrize("name", ["fa", "rnd"])
def test_sampled_queries_every_product(gpu, inputs, oracles, name, w, rc):
    """seq.kmer.pos(.rc) = the unsampled rows filtered by (query mask, index mask), in order, for a
    self query, a mutated copy and an unrelated query; segments, blocks, chains and the raster are
    the CPU references applied to those rows; max.occ on top (counting a k-mer's occurrences in
    the sampled index, which holds nothing else) gives the rows under both."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    s, k = inputs[name]
    ox, qs, rows = oracles[name]
    imask = minimizer_ref.mask(s, k, w)
    idx = DeviceIndex.build(_seq_t(torch, s), k, w=w)
    assert idx.sampling == w
    L = len(s)
    frames = [(1, 1, 64, 64, (L + 63) // 64, (L + 63) // 64), (100, 50, 7, 333, 30, 10)]
    for qn, q in qs.items():
        fwd = rc_host(q) if rc else q                # the strand the rule runs on
        qmask = minimizer_ref.mask(fwd, k, w)
        assert np.array_equal(qmask, minimizer_ref.mask(q, k, w, rc))
        want = minimizer_ref.filter_rows(rows[qn, rc], k, qmask, imask)
        if qn != "unrelated" and not rc:             # (the strands share few minimizers: rc may be empty)
            assert 0 < len(want) < len(rows[qn, rc])
        t = _seq_t(torch, q)
        _check_products(torch, idx, t, k, rc, want, frames if qn == "self" else frames[:1])
        if qn == "self":
            idx.set_max_occ(3)
            both = want[_sampled_occurrences(ox, imask)[want[:, 1]] <= 3]
            assert rc or (len(both) and (name != "fa" or len(both) < len(want)))
            dq = idx.query_rc(t, k) if rc else idx.query(t, k)
            assert np.array_equal(_rows(dq), both)
            idx.set_max_occ(0)
    idx.free()


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
def test_range_entries_cut_through_spans(gpu, inputs, oracles, rc):
    """[w0, w1) selects over the whole sequence and masks the range: the whole query's rows
    restricted to it, also where the range's edges fall inside spans and tiles."""
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex, runs_expand
    s, k = inputs["fa"]
    ox, qs, rows = oracles["fa"]
    w = 19
    imask = minimizer_ref.mask(s, k, w)
    idx = DeviceIndex.build(_seq_t(torch, s), k, w=w)
    q = qs["mutated"]
    want = minimizer_ref.filter_rows(rows["mutated", rc], k, minimizer_ref.mask(q, k, w, rc), imask)
    t = _seq_t(torch, q)
    nw = len(q) - k + 1
    rng_q = idx.query_range_rc if rc else idx.query_range
    rng_r = idx.query_range_runs_rc if rc else idx.query_range_runs
    for w0, w1 in ((0, nw), (13, nw - 3), (TILE - 7, TILE + 9), (TILE + 3, nw), (100, 100)):
        i = want[:, 0].astype(np.int64)
        sub = want[(i > w0 + k - 1) & (i <= w1 + k - 1)]
        assert np.array_equal(_rows(rng_q(t, k, w0, w1)), sub), (w0, w1)
        kind, tt, h = rng_r(t, k, w0, w1)
        assert h == len(sub)
        if kind == "rows":
            got = tt.cpu().numpy()[:h]
        else:
            out = torch.full((h, 2), -1, dtype=torch.int32, device="cuda")
            runs_expand(tt, h, out)
            got = out.cpu().numpy()
        assert np.array_equal(got, sub), (w0, w1, kind)
    idx.free()


def test_another_k_queries_as_on_an_unsampled_index(gpu, inputs):
    """A query at a k other than the index's launches what it launches on an unsampled index: no
    selection of the query, no mask pass."""
    torch = gpu
    from kmer_hasher_amd import device as D
    s, k = inputs["fa"]
    t = _seq_t(torch, s)
    a, b = D.DeviceIndex.build(t, k, w=5), D.DeviceIndex.build(t, k)
    D.timing_enable(True)
    try:
        D.timing_reset()
        _rows(a.query(t, k - 1))
        ka = {n for n, v in D.timing_report().items() if v[0]}
        D.timing_reset()
        _rows(b.query(t, k - 1))
        kb = {n for n, v in D.timing_report().items() if v[0]}
    finally:
        D.timing_enable(False)
    assert ka == kb and "k_query_probe" in ka, (ka, kb)
    a.free()
    b.free()


def test_pairs_of_two_sampled_indexes(gpu, inputs):
    from kmer_hasher_amd import kmer_pairs, make_kmer_hash
    s, k = inputs["fa"]
    other = _mutated(s, 8)
    wa, wb = 5, 19
    pa, pb = make_kmer_hash(s, k, False, wa), make_kmer_hash(other, k, False, wb)
    got = kmer_pairs(pa, pb)
    ma, mb = minimizer_ref.mask(s, k, wa), minimizer_ref.mask(other, k, wb)
    want = pairs_ref.cross(_masked_starts(s, k, ma), _masked_starts(other, k, mb)).reshape(-1, 2)
    assert len(want) and np.array_equal(got, want)
    pa.free()
    pb.free()


def _masked_starts(s, k, m):
    """pairs_ref.kmer_starts without the unselected starts; keys by first selected start."""
    d = {key: [x for x in st if m[x - 1]] for key, st in pairs_ref.kmer_starts(s, k).items()}
    d = {key: st for key, st in d.items() if st}
    return dict(sorted(d.items(), key=lambda kv: kv[1][0]))


# ------------------------------------------------------------------ 4. refusals and launches
def test_refusals(gpu, test_lib, monkeypatch, inputs):
    torch = gpu
    from kmer_hasher_amd import KmerHashError, make_kmer_hash, seq_kmer_pos
    from kmer_hasher_amd import _lib
    from kmer_hasher_amd.device import DeviceIndex
    s, k = inputs["fa"]
    t = _seq_t(torch, s)
    for w in (0, 257, -3):
        with pytest.raises(Exception, match="w must be between 1 and 256"):
            DeviceIndex.build(t, k, w=w)
    # no sampled part builds: the part entry has no w, and the plan refuses one
    p = DeviceIndex.build_part(t, k, 0, 2)
    assert p.sampling == 1
    p.free()
    ptr = make_kmer_hash(s, k, False, 5)
    monkeypatch.setenv("KMHG_DEVICES", "0,0")
    with pytest.raises(KmerHashError, match="a sampled index is queried on its own device"):
        seq_kmer_pos(ptr, s, k)
    monkeypatch.delenv("KMHG_DEVICES")
    assert len(seq_kmer_pos(ptr, s, k))
    ptr.free()
    monkeypatch.setenv("KMHG_BUILD", "v1")
    with pytest.raises(KmerHashError, match="a sampled index needs the partitioned build"):
        make_kmer_hash(s, k, False, 5)


def test_timing_names_the_new_pass_and_not_the_diagonal_path(gpu, inputs):
    torch = gpu
    from kmer_hasher_amd import device as D
    s, k = inputs["fa"]
    t = _seq_t(torch, s)
    plain, sampled = D.DeviceIndex.build(t, k), D.DeviceIndex.build(t, k, w=5)
    _rows(plain.query(t, k))                         # (the diagonal path's preparation, once)
    D.timing_enable(True)
    try:
        D.timing_reset()
        _rows(plain.query(t, k))
        k0 = {n for n, v in D.timing_report().items() if v[0]}
        D.timing_reset()
        _rows(sampled.query(t, k))
        k1 = {n for n, v in D.timing_report().items() if v[0]}
        D.timing_reset()
        sampled.segments(t, k)
        k2 = {n for n, v in D.timing_report().items() if v[0]}
    finally:
        D.timing_enable(False)
    new = {"k_minimizer_mask", "k_qrec_minmask"}
    assert "k_query_probe" in k0 and not (new & k0), k0
    assert new <= k1 and "k_query_probe" in k1, k1
    assert not ({"k_diag_valid", "k_diag_prep"} & k1), k1
    assert k1 - new <= k0, (k0, k1)
    assert new <= k2, k2
    assert sampled.info()["n_positions"] < plain.info()["n_positions"]
    plain.free()
    sampled.free()


def test_get_sampling_is_1_on_counts_and_suffix_hash_indexes(gpu, tmp_path):
    from kmer_hasher_amd import count_kmers, count_kmers_fq_sh_rp, get_sampling
    c = count_kmers([_iid(300, 4)], (11, 0, 1))
    assert get_sampling(c) == 1
    fq = tmp_path / "r.fq"
    s = _iid(120, 6)
    fq.write_text("".join(f"@r{i}\n{s[i:i + 60]}\n+\n{'I' * 60}\n" for i in range(40)))
    sh = count_kmers_fq_sh_rp(str(fq), (11, 4, 0, 1, 1000, 1 << 20, 1, 0))
    assert get_sampling(sh) == 1


def test_nothing_selected_builds_an_empty_index(gpu):
    """w longer than every run of indexable windows: no span, no selected window, an index with
    no k-mer that every reader takes."""
    torch = gpu
    from kmer_hasher_amd import kmer_pos, make_kmer_hash, seq_kmer_pos
    k, w = 15, 19
    s = list(_iid(5000, 8))
    s[::20] = "N" * len(s[::20])                     # runs of 19 chars: 5 windows each, < w
    s = "".join(s)
    assert not minimizer_ref.mask(s, k, w).any() and minimizer_ref.valid(s, k).any()
    ptr = make_kmer_hash(s, k, False, w)
    inf = ptr.info()
    assert inf.n_kmers == 0 and inf.n_positions == 0
    got = kmer_pos(ptr, 15)
    assert got["kmer"] == [] and len(got["pos"]) == 0 and len(got["count"]) == 0
    assert len(seq_kmer_pos(ptr, s, k)) == 0
    ptr.free()
