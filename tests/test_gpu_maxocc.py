"""kmer.max.occ (kmhg_set_max_occ; k_qrec_mask of kmhg_kernels.hip): with a cap of n set on a
position index, a query window whose k-mer occurs at more than n positions of the index yields no
hit, in every product of the query.  The checker is tests/maxocc_ref.py's mask_rows on the
clean-room oracle's rows, fed to segs_ref / blocks_ref / chains_ref / raster_ref.  Integer work:
every comparison is exact, order included.  The pass walks tiles of 2,048 windows between the
probe and the scan of its tile totals, so the shapes have more than one tile, a tile whose
multi-hit windows are all masked, and counts on both sides of every cap."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import blocks_ref
import chains_ref
import maxocc_ref
import raster_ref
import segs_ref

pytestmark = pytest.mark.gpu

M = 2**31 - 1
TILE = 2048
CAPS = [0, 1, 2, 4, 5, 256, 2100, M]
MSG = "max.occ must be between 0 and 2^31-1"


def _seq_t(torch, s):
    a = np.frombuffer(s.encode("latin-1"), np.uint8) if isinstance(s, str) else s
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _index(torch, s, k):
    from kmer_hasher_amd.device import DeviceIndex
    return DeviceIndex.build(_seq_t(torch, s), k)


def _rows(q):
    r = q.rows().cpu().numpy()
    q.free()
    return r


def _runs_rows(torch, got):
    """A runs entry's answer as rows."""
    from kmer_hasher_amd.device import runs_expand
    kind, t, h = got
    if kind == "rows":
        return t.cpu().numpy()[:h]
    out = torch.full((h, 2), -1, dtype=torch.int32, device="cuda")
    runs_expand(t, h, out)
    return out.cpu().numpy()


def _window_rows(rows, k, w0, w1):
    """The rows of windows [w0, w1): i is the window's 1-based end, w + k."""
    i = rows[:, 0].astype(np.int64)
    return rows[(i > w0 + k - 1) & (i <= w1 + k - 1)]


def _check_products(torch, idx, t, k, rc, want, frames=(), max_gap=None, chains=((5000, 500, 1),)):
    """Every product of the query `t` on `idx` (its cap set by the caller) against the references
    of `want`, the oracle's rows after masking."""
    dq = idx.query_rc(t, k) if rc else idx.query(t, k)
    assert dq.n_rows == len(want)
    assert np.array_equal(dq.rows().cpu().numpy(), want)
    segs = segs_ref.segments(want)
    for ml in (1, 2):
        got, h = idx.segments(t, k, ml, rc=rc)
        ws = segs[segs[:, 2] >= ml]
        assert h == len(want) and got.shape == ws.shape and np.array_equal(got.cpu().numpy(), ws)
        assert torch.equal(got, dq.segments(ml)), ("segments: the two routes", ml)
    g = k if max_gap is None else max_gap
    for gap, ml, mh in ((g, 1, 1), (0, 2, 2)):
        got, h = idx.blocks(t, k, gap, ml, mh, rc=rc)
        wb = blocks_ref.merge(segs[segs[:, 2] >= ml], gap, mh)
        assert h == len(want) and got.shape == wb.shape and np.array_equal(got.cpu().numpy(), wb)
        assert torch.equal(got, dq.blocks(gap, ml, mh)), ("blocks: the two routes", gap, ml, mh)
    wb = blocks_ref.merge(segs, g, 1)
    for p in chains:
        wc, wm = chains_ref.chains(wb, *p)
        for rf in (False, True):
            c, b, m, h = idx.chains(t, k, p[0], p[1], g, 1, p[2], rc=rc, row_free=rf)
            assert h == len(want), (rf, h)
            assert b.shape == wb.shape and np.array_equal(b.cpu().numpy(), wb), rf
            assert c.shape == wc.shape and np.array_equal(c.cpu().numpy(), wc), rf
            assert np.array_equal(m.cpu().numpy(), wm), rf
    for f in frames:
        got, h = idx.raster(t, k, f, rc=rc)
        assert h == len(want)
        assert np.array_equal(got.cpu().numpy(), raster_ref.raster(want, f)), f
        assert torch.equal(got, dq.raster(f)), ("raster: the two routes", f)
    dq.free()


# ------------------------------------------------------------------ 1. counted index
@pytest.fixture(scope="module")
def counted():
    """maxocc_ref.counted_case with the oracle's rows, and the rows after every cap, once."""
    k, units, a, q, ox = maxocc_ref.counted_case()
    rows = ox.query(q, k).reshape(-1, 2)
    per_window = np.unique(rows[:, 0], return_counts=True)[1]
    assert set(per_window.tolist()) == set(maxocc_ref.COUNTS)
    nw = len(q) - k + 1
    assert TILE < nw < 2 * TILE and rows[-1, 0] == len(q)
    masked = {n: maxocc_ref.mask_rows(a, k, rows, n, ox) for n in CAPS}
    # a cap of 4: the second tile's multi-hit windows (5 and 2,100 hits) all go, its single hits stay
    second = _window_rows(masked[4], k, TILE, nw)
    assert len(second) == 6 and len(np.unique(second[:, 0])) == 6
    assert len(_window_rows(rows, k, TILE, nw)) == 6 + 6 * 5 + 2100
    return k, a, q, ox, rows, masked


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("cap", CAPS)
def test_counted_index_every_entry(gpu, counted, cap, rc):
    """Units of 1, 2, 4, 5, 255, 257 and 2,100 hits under caps on both sides of each.  The reverse
    strand is given rc(query), whose reverse complement is the query: the same rows through the
    reverse stage."""
    torch = gpu
    k, a, q, ox, rows, masked = counted
    want = masked[cap]
    assert (len(want) == len(rows)) == (cap == 0 or cap >= 2100)
    idx = _index(torch, a, k)
    assert idx.set_max_occ(cap) is idx and idx.max_occ == cap
    t = _seq_t(torch, rc_host(q) if rc else q)
    nw = len(q) - k + 1
    frames = [(1, 1, 64, 1024, 45, 54), (100, 50, 7, 333, 300, 100)]
    _check_products(torch, idx, t, k, rc, want, frames)
    # a range whose first window is no multiple of 2,048 or of 8, ending inside the second tile
    rng_q = idx.query_range_rc if rc else idx.query_range
    rng_r = idx.query_range_runs_rc if rc else idx.query_range_runs
    for w0, w1 in ((0, nw), (13, nw - 3), (21, 22), (TILE + 3, nw)):
        sub = _window_rows(want, k, w0, w1)
        assert np.array_equal(_rows(rng_q(t, k, w0, w1)), sub), (w0, w1)
        got = rng_r(t, k, w0, w1)
        assert got[2] == len(sub)
        assert np.array_equal(_runs_rows(torch, got), sub), (w0, w1, got[0])
    idx.free()


# ------------------------------------------------------------------ 2. test.fa self
@pytest.fixture(scope="module")
def fa(testfa):
    s = testfa[:6000]
    ox = O.OracleIndex(s, 15)
    fwd = ox.query(s, 15).reshape(-1, 2)
    rev = ox.query(rc_host(s), 15).reshape(-1, 2)
    assert len(fwd) == 5_275_316
    return s, ox, fwd, rev


@pytest.mark.parametrize("rc", [False, True], ids=["fwd", "rc"])
@pytest.mark.parametrize("cap", [1, 8])
def test_testfa_self(gpu, fa, cap, rc):
    torch = gpu
    s, ox, fwd, rev = fa
    want = maxocc_ref.mask_rows(s, 15, rev if rc else fwd, cap, ox)
    assert rc or 0 < len(want) < 200
    idx = _index(torch, s, 15).set_max_occ(cap)
    _check_products(torch, idx, _seq_t(torch, s), 15, rc, want)
    idx.free()


# ------------------------------------------------------------------ 3. beyond 2^31 rows
def test_homopolymer_unique_only(gpu):
    """ "A" * 47000 against itself at k = 15: 46,986 windows of 46,986 hits each.  Without a cap the
    runs entry refuses the 2,207,684,196 rows; with a cap of 1 nothing is left anywhere."""
    torch = gpu
    from kmer_hasher_amd import _lib
    n, k = 47000, 15
    nw = n - k + 1
    s = "A" * n
    idx = _index(torch, s, k)
    t = _seq_t(torch, s)
    with pytest.raises(_lib.KmhgError, match=r"more than 2\^31-1 rows"):
        idx.query_range_runs(t, k, 0, nw)
    idx.set_max_occ(1)
    dq = idx.query(t, k)
    assert dq.n_rows == 0
    dq.free()
    kind, r, h = idx.query_range_runs(t, k, 0, nw)
    assert h == 0
    g, h = idx.segments(t, k)
    assert h == 0 and tuple(g.shape) == (0, 3)
    f = (1, 1, 512, 512, 92, 92)
    m, h = idx.raster(t, k, f)
    assert h == 0 and tuple(m.shape) == (92, 92) and int(m.abs().sum()) == 0
    idx.set_max_occ(nw - 1)                           # one short of the count: still nothing
    g, h = idx.segments(t, k)
    assert h == 0 and len(g) == 0
    idx.set_max_occ(0)
    g, h = idx.segments(t, k)
    assert h == nw * nw == 2_207_684_196 and len(g) == 2 * nw - 1 == 93_971
    idx.free()


# ------------------------------------------------------------------ 4. off means off
def test_off_launches_nothing_new(gpu, counted):
    torch = gpu
    from kmer_hasher_amd import device as D
    k, a, q, ox, rows, masked = counted
    idx = _index(torch, a, k)
    t = _seq_t(torch, q)
    _rows(idx.query(t, k))                            # the index's first query prepares it
    D.timing_enable(True)
    try:
        D.timing_reset()
        off = _rows(idx.query(t, k))
        g, _ = idx.segments(t, k)
        k0 = {n for n, v in D.timing_report().items() if v[0]}
        idx.set_max_occ(3)
        D.timing_reset()
        on = _rows(idx.query(t, k))
        k1 = {n for n, v in D.timing_report().items() if v[0]}
        D.timing_reset()
        idx.segments(t, k)
        k2 = {n for n, v in D.timing_report().items() if v[0]}
    finally:
        D.timing_enable(False)
    assert "k_query_probe" in k0 and "k_scan_tiles_u64" in k0 and "k_qrec_mask" not in k0, k0
    assert "k_qrec_mask" in k1 and k1 - {"k_qrec_mask"} <= k0, (k0, k1)
    assert "k_qrec_mask" in k2 and "k_query_probe" in k2, k2
    assert np.array_equal(off, rows)
    assert np.array_equal(on, maxocc_ref.mask_rows(a, k, rows, 3, ox))
    idx.free()


# ------------------------------------------------------------------ 5. the setter
def test_setter(gpu, counted):
    torch = gpu
    from kmer_hasher_amd import _lib, api
    from kmer_hasher_amd.device import DeviceIndex
    k, a, q, ox, rows, masked = counted
    L = _lib.lib()
    idx = _index(torch, a, k)
    t = _seq_t(torch, q)
    assert idx.max_occ == 0
    for n in (1, 7, M, 0):
        idx.set_max_occ(n)
        assert idx.max_occ == n
    idx.set_max_occ(5)
    for bad in (-1, -2**63, M + 1, 2**63 - 1):
        with pytest.raises(_lib.KmhgError) as e:
            idx.set_max_occ(bad)
        assert str(e.value) == MSG and e.value.code == _lib.KMHG_EINVAL
        assert idx.max_occ == 5                       # a refused value changes nothing
    assert L.kmhg_set_max_occ(None, 1) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "null index"
    assert L.kmhg_get_max_occ(idx.handle, None) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "null argument"
    # the next query on the same index follows the setting, no rebuild
    assert np.array_equal(_rows(idx.query(t, k)), masked[5])
    idx.set_max_occ(2)
    assert np.array_equal(_rows(idx.query(t, k)), masked[2])
    idx.set_max_occ(0)
    assert np.array_equal(_rows(idx.query(t, k)), rows)
    # kmer.pos and kmer.pairs do not look at it
    other = _index(torch, q, k)
    opt = api.OPT_POS | api.OPT_PAIRS | api.OPT_COUNT | api.OPT_KMER

    def readout():
        out = {n: v.cpu().numpy().tobytes() for n, v in idx.positions(opt).items()}
        qh, n = C.c_void_p(), C.c_int64()
        _lib.check(L.kmhg_pairs_run(idx.handle, other.handle, C.byref(qh), C.byref(n)))
        pairs = np.empty((n.value, 2), np.int32)
        _lib.check(L.kmhg_query_fill(qh, pairs.ctypes.data_as(C.c_void_p)))
        L.kmhg_query_free(qh)
        assert n.value > 0
        out["pairs"] = pairs.tobytes()
        return out

    before = readout()
    idx.set_max_occ(1)
    other.set_max_occ(1)
    assert readout() == before
    other.free()
    idx.free()
    # a counts index and a suffix-hash index are refused; the host API carries the same words
    cp = api.count_kmers("ACGTACGTACGTAAACCC", (4, 0, 1))
    sh = api.count_kmers_fq_sh_rp("no-such-file.fq", [15, 10, 0, 1, -1, 1, 1, 0])
    assert L.kmhg_set_max_occ(cp.handle, 2) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "max.occ needs a position index"
    assert L.kmhg_set_max_occ(sh.handle, 2) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "External pointer has incorrect tag"
    with pytest.raises(api.KmerHashError, match="max.occ needs a position index"):
        api.set_max_occ(cp, 2)
    with pytest.raises(api.KmerHashError, match="External pointer has incorrect tag"):
        api.set_max_occ(sh, 2)
    cp.free()
    sh.free()
    ptr = api.make_kmer_hash(a, k)
    assert api.get_max_occ(ptr) == 0 and api.set_max_occ(ptr, 4) == 0 and api.get_max_occ(ptr) == 4
    with pytest.raises(api.KmerHashError) as e:
        api.set_max_occ(ptr, -1)
    assert str(e.value) == MSG
    assert np.array_equal(api.seq_kmer_pos(ptr, q, k), masked[4])
    assert np.array_equal(api.seq_kmer_pos_rc(ptr, rc_host(q), k), masked[4])
    segs = segs_ref.segments(masked[4])
    for rf in (False, True):
        assert np.array_equal(api.seq_kmer_segs(ptr, q, k, row_free=rf), segs)
    assert api.set_max_occ(ptr) == 4 and api.get_max_occ(ptr) == 0          # the default is off
    assert np.array_equal(api.seq_kmer_pos(ptr, q, k), rows)
    ptr.free()
    # a part takes the setting; part indices are for the part entry only
    part = DeviceIndex.build_part(_seq_t(torch, a), k, 0, 2)
    assert part.set_max_occ(9).max_occ == 9
    part.free()


# ------------------------------------------------------------------ 6. KMHG_DEVICES
def test_devices_replicas_take_the_home_value_on_every_call(gpu, test_lib, monkeypatch, counted):
    from kmer_hasher_amd import api
    k, a, q, ox, rows, masked = counted
    monkeypatch.setenv("KMHG_DEVICES", "0,0")
    monkeypatch.setenv("KMHG_TEST_REPLICA", "1")      # the second part runs on a copy of the index
    ptr = api.make_kmer_hash(a, k)
    assert np.array_equal(api.seq_kmer_pos(ptr, q, k), rows)         # the copy exists from here on
    api.set_max_occ(ptr, 4)
    got = api.seq_kmer_pos(ptr, q, k)
    monkeypatch.delenv("KMHG_DEVICES")
    single = api.seq_kmer_pos(ptr, q, k)
    assert np.array_equal(single, masked[4]) and np.array_equal(got, single)
    monkeypatch.setenv("KMHG_DEVICES", "0,0")
    api.set_max_occ(ptr, 0)
    assert np.array_equal(api.seq_kmer_pos(ptr, q, k), rows)
    ptr.free()


# ------------------------------------------------------------------ 7. a part index
def test_part_query_honours_the_cap(gpu, counted):
    torch = gpu
    from kmer_hasher_amd.device import DeviceIndex
    k, a, q, ox, rows, masked = counted
    ta, t = _seq_t(torch, a), _seq_t(torch, q)
    nt = (len(q) - k + 1 + TILE - 1) // TILE
    for cap in (0, 4):
        got = []
        for p in range(2):
            part = DeviceIndex.build_part(ta, k, p, 2).set_max_occ(cap)
            dq = part.query_part(t, k)
            off = dq.tile_offsets().cpu().numpy()
            assert len(off) == nt + 1 and off[0] == 0 and off[-1] == dq.n_rows
            assert (np.diff(off.astype(np.int64)) >= 0).all()
            got.append(_rows(dq))
            part.free()
        assert cap or (len(got[0]) and len(got[1]))
        both = np.concatenate(got)
        merged = both[np.argsort(both[:, 0], kind="stable")]     # a window's rows: one part, j order
        assert np.array_equal(merged, masked[cap]), cap
