"""seq.kmer.raster -- (i, j) rows binned into a count matrix (kmhg_rows_raster, kmhg_query_raster
and the row-free kmhg_raster_run_device; kmhg_raster.hip) -- against tests/raster_ref.py, the
numpy restatement of the definition in include/kmhgpu.h, computed from crafted rows or from the
clean-room oracle's rows.  Integer work: every comparison is exact.  The implementation has one
path per route (no light-tile kernel, no LDS-private matrix), so there is no selector to straddle;
the shapes below sit around the wave (64), the workgroup (256) and the tile (2,048)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from revcomp_ref import rc_host
import raster_ref
from test_gpu_query_rc import _spliced

pytestmark = pytest.mark.gpu

M = 2**31 - 1
TILE = 2048
BLOCK = 256
EMIT_DIRECT = 4


def _dev(torch, rows):
    r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 2))
    return torch.from_numpy(r).cuda()


def _rows_raster(torch, t, frame):
    from kmer_hasher_amd import device
    got = device.rows_raster(t, frame)
    assert got.dtype == torch.int64 and tuple(got.shape) == (frame[4], frame[5]) and got.is_cuda
    return got.cpu().numpy()


def _check_rows(torch, rows, frames):
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    t = _dev(torch, rows)
    out = []
    for f in frames:
        want = raster_ref.raster(rows, f)
        got = _rows_raster(torch, t, f)
        assert np.array_equal(got, want), (len(rows), f)
        out.append(want)
    return out


# ------------------------------------------------------------------ 1. rows route, one diagonal
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_rows_one_diagonal(gpu, n):
    """Rows (t + 3, t + 5): frames start above 1 and their n_i cuts the tail off, so rows fall
    outside on every side; width 2^20 puts every row of the frame into one cell."""
    t = np.arange(n, dtype=np.int64)
    rows = np.stack([t + 3, t + 5], axis=1)
    frames = []
    for bi in (1, 7, 64, 2**20):
        for bj in (1, 7, 64, 2**20):
            n_i = 1 if bi == 2**20 else max(1, (n - 40) // bi)
            n_j = 1 if bj == 2**20 else max(1, (n + 30) // bj)
            frames.append((10, 9, bi, bj, n_i, n_j))
    got = _check_rows(gpu, rows, frames)
    assert int(got[-1][0, 0]) == max(n - 7, 0)       # i >= 10: all but the first 7 rows, one cell


# ------------------------------------------------------------------ 2. wave-aggregation shapes
def test_rows_cell_changes_at_lane_and_tile_edges(gpu):
    """Runs of 64 and of 2,048 equal cells: the cell changes exactly between lane 63 and 64, and
    between two tiles; then the same shifted by one row."""
    n = 2 * TILE + 64
    t = np.arange(n, dtype=np.int64)
    for shift in (0, 1, 63):
        rows = np.stack([t + 1 + shift, t + 1 + shift], axis=1)
        _check_rows(gpu, rows, [(1, 1, 64, 64, 70, 70), (1, 1, TILE, TILE, 3, 3),
                                (1, 1, 64, TILE, 66, 3), (1, 1, BLOCK, 1, 17, 4096)])


def test_rows_alternating_cells(gpu):
    """No two neighbouring rows share a cell."""
    n = TILE + 77
    t = np.arange(n, dtype=np.int64)
    rows = np.stack([1 + (t % 2) * 100, 1 + (t // 2)], axis=1)
    a, = _check_rows(gpu, rows, [(1, 1, 100, 2**20, 2, 1)])
    assert a[:, 0].tolist() == [(n + 1) // 2, n // 2]
    _check_rows(gpu, rows, [(1, 1, 1, 1, 101, 1100), (1, 1, 50, 3, 3, 400)])


def test_rows_one_window_with_5000_hits(gpu):
    rows = np.stack([np.full(5000, 5), np.arange(1, 5001)], axis=1)
    one, = _check_rows(gpu, rows, [(1, 1, 2**20, 2**20, 1, 1)])
    assert one.tolist() == [[5000]]
    _check_rows(gpu, rows, [(5, 1, 1, 1, 1, 5000), (1, 1, 5, 64, 2, 79), (6, 1, 1, 1, 4, 5000),
                            (1, 100, 3, 7, 5, 600)])


def test_rows_unsorted_equal_sorted(gpu):
    rng = np.random.default_rng(5)
    n = 3 * TILE + 11
    rows = np.stack([rng.integers(1, 400, n), rng.integers(1, 400, n)], axis=1)
    rows = np.unique(rows, axis=0)
    perm = np.random.default_rng(6).permutation(len(rows))
    frames = [(1, 1, 1, 1, 400, 400), (7, 3, 13, 5, 20, 70), (1, 1, 2**20, 2**20, 1, 1)]
    a = _check_rows(gpu, rows, frames)
    b = _check_rows(gpu, rows[perm], frames)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_rows_below_the_frame_and_extreme_values(gpu):
    """i or j below the frame (0 and negatives too: no i, j >= 1 check) and the value 2^31 - 1."""
    rows = [(1, 1), (0, 5), (5, 0), (-1, -1), (-2**31, 7), (7, -2**31), (9, 9), (M, M), (M, 1),
            (1, M), (M - 1, M), (10, 8), (8, 10)]
    got = _check_rows(gpu, rows, [(1, 1, M, M, 1, 1), (M, M, 1, 1, 1, 1), (M - 1, 1, 1, M, 2, 1),
                                  (9, 9, 1, 1, 2, 2), (1, 1, 2**29, 2**29, 3, 3),
                                  (M, 7, 1, 1, 1, 1), (7, M, 1, 1, 1, 1), (2, 2, 3, 3, 3, 3)])
    assert got[0].tolist() == [[8]] and got[1].tolist() == [[1]]
    # (-2^31, 7) and (7, -2^31) are not taken for a coordinate one above 2^31 - 1
    assert got[5].tolist() == [[0]] and got[6].tolist() == [[0]]


# ------------------------------------------------------------------ 3. row-free route, oracle rows
def _index(torch, s, k):
    from kmer_hasher_amd.device import DeviceIndex
    a = np.frombuffer(s.encode(), np.uint8) if isinstance(s, str) else s
    return DeviceIndex.build(torch.from_numpy(np.ascontiguousarray(a)).cuda(), k)


def _seq_t(torch, s):
    a = np.frombuffer(s.encode(), np.uint8) if isinstance(s, str) else s
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _check_free(torch, idx, q, kq, rc, want_rows, frames):
    t = _seq_t(torch, q)
    for f in frames:
        got, h = idx.raster(t, kq, f, rc=rc)
        assert h == len(want_rows), (h, len(want_rows))
        assert np.array_equal(got.cpu().numpy(), raster_ref.raster(want_rows, f)), (f, rc)


@pytest.fixture(scope="module")
def testfa_rows(testfa):
    s = testfa[:6000]
    ox = O.OracleIndex(s, 15)
    fwd = ox.query(s, 15).reshape(-1, 2)
    rev = ox.query(rc_host(s), 15).reshape(-1, 2)
    assert len(fwd) == 5_275_316
    return s, fwd, rev


TESTFA_FRAMES = [(1, 1, 6, 6, 1000, 1000),           # bins (1000, 1000) over 1..6000
                 (2000, 1000, 1, 3, 512, 700),       # width 1 in a cropped frame
                 (1, 4500, 2, 2, 750, 750)]          # an off-diagonal corner only


@pytest.mark.parametrize("rc", [False, True])
def test_row_free_testfa_self(gpu, testfa_rows, rc):
    s, fwd, rev = testfa_rows
    idx = _index(gpu, s, 15)
    _check_free(gpu, idx, s, 15, rc, rev if rc else fwd, TESTFA_FRAMES)


def test_row_free_spliced_n_and_other_query_k(gpu):
    """Inverted segments and N runs, both strands; then a query k that is not the index k (table
    probes: the diagonal path needs equal k)."""
    s, a = _spliced(6000, 41, 15)
    s = s.copy()
    s[1000:1003] = ord("N")
    s[2047] = ord("n")
    s[5000:5100] = ord("N")
    idx = _index(gpu, a, 15)
    frames = [(1, 1, 6, 6, 1000, 1000), (300, 300, 1, 1, 900, 1100), (1, 1, 2**20, 2**20, 1, 1)]
    ox = O.OracleIndex(a, 15)
    for rc in (False, True):
        want = ox.query(rc_host(s) if rc else s, 15).reshape(-1, 2)
        assert len(want) > 600
        _check_free(gpu, idx, s, 15, rc, want, frames)
    idx12 = _index(gpu, a, 12)
    want = O.OracleIndex(a, 12).query(s, 15).reshape(-1, 2)
    _check_free(gpu, idx12, s, 15, False, want, frames)


# ------------------------------------------------------------------ 4. window-count boundaries
COUNTS = [1, 2, EMIT_DIRECT, EMIT_DIRECT + 1, BLOCK - 1, BLOCK + 1, TILE + 52]


def _units(k):
    rng = np.random.default_rng(123)
    return ["".join(rng.choice(list("ACGT"), k + 5)) for _ in COUNTS]


@pytest.fixture(scope="module")
def counted_index():
    """Each unit (k + 5 chars: 6 windows) repeated c times, copies separated by N: a query window
    of the unit has exactly c hits."""
    k = 15
    units = _units(k)
    a = "".join((u + "N") * c for u, c in zip(units, COUNTS))
    return k, units, a, O.OracleIndex(a, k)


@pytest.mark.parametrize("nw", [TILE - 1, TILE, TILE + 1])
def test_row_free_window_counts(gpu, counted_index, nw):
    from kmer_hasher_amd import synth
    k, units, a, ox = counted_index
    head = "N".join(units) + "N"
    tail = "N" + units[3] + units[6][:k]             # hits in the last windows too
    L = nw + k - 1
    fill = synth.iid(L - len(head) - len(tail), 900 + nw).tobytes().decode()
    q = head + fill + tail
    assert len(q) == L
    want = ox.query(q, k).reshape(-1, 2)
    per_window = np.unique(want[:, 0], return_counts=True)[1]
    assert set(COUNTS) <= set(per_window.tolist())
    idx = _index(gpu, a, k)
    La = len(a)
    frames = [(1, 1, 8, 64, -(-L // 8), -(-La // 64)), (1, 1, 1, 2**20, L, 1),
              (1, 1, 2**20, 1, 1, La), (20, 400, 3, 5, 40, 9000), (L - 30, 1, 1, 7, 40, 8000)]
    _check_free(gpu, idx, q, k, False, want, frames)


def test_row_free_no_hit(gpu):
    from kmer_hasher_amd import synth
    a = synth.iid(3000, 17)
    q = "T" * 3000
    assert len(O.OracleIndex(a, 15).query(q, 15)) == 0
    idx = _index(gpu, a, 15)
    got, h = idx.raster(_seq_t(gpu, q), 15, (1, 1, 3, 3, 1000, 1000))
    assert h == 0 and int(got.abs().sum()) == 0
    got, h = idx.raster(_seq_t(gpu, q), 15, (1, 1, 3, 3, 1000, 1000), rc=True)
    assert h == 0 and int(got.abs().sum()) == 0


# ------------------------------------------------------------------ 5. route agreement
def test_routes_agree_and_runs_repeat(gpu):
    torch = gpu
    from kmer_hasher_amd import device
    s, a = _spliced(5000, 7, 15)
    idx = _index(torch, a, 15)
    t = _seq_t(torch, s)
    for rc in (False, True):
        for f in [(1, 1, 5, 5, 1000, 1000), (100, 200, 1, 1, 2000, 2000), (1, 1, 5000, 5000, 1, 1)]:
            buf1 = torch.empty(f[4] * f[5], dtype=torch.int32, device="cuda")
            buf2 = torch.full((f[4] * f[5],), -1, dtype=torch.int32, device="cuda")
            free1, h1 = idx.raster(t, 15, f, rc=rc, out=buf1)
            free2, h2 = idx.raster(t, 15, f, rc=rc, out=buf2)
            assert h1 == h2 and torch.equal(buf1, buf2)          # the same bytes on every run
            q = idx.query_rc(t, 15) if rc else idx.query(t, 15)
            assert q.n_rows == h1
            by_query = q.raster(f)
            by_rows = device.rows_raster(q.rows(), f)
            assert torch.equal(free1, by_query) and torch.equal(free1, by_rows)
            assert int(free1.sum()) == raster_ref.in_frame(q.rows().cpu().numpy(), f)
            q.free()


# ------------------------------------------------------------------ 6. beyond 2^31 rows
def test_more_than_2_31_rows(gpu):
    """Index and query "A" * 47000 at k = 15: each of 46,986 windows hits 46,986 positions,
    2,207,684,196 rows.  The raster counts them: every (i, j) with 15 <= i <= 47000 and
    1 <= j <= 46986 is a row, so a cell holds (its i's) x (its j's).
    The refusal "result has more than 2^31-1 rows" is the runs entry's
    (kmhg_query_run_device_range_runs, the form rows leave a device in), which is asserted here;
    DeviceIndex.query itself does not refuse -- it writes the 17.7 GB of rows into device memory,
    and the host entries then refuse them as "2^31-1 columns" (tests/test_gpu_boundary.py).
    Measured on an MI355X: 0.22 s, index build and host check included."""
    torch = gpu
    from kmer_hasher_amd import _lib
    n, k = 47000, 15
    nw = n - k + 1
    s = "A" * n
    idx = _index(torch, s, k)
    t = _seq_t(torch, s)
    with pytest.raises(_lib.KmhgError, match="result has more than 2\\^31-1 rows") as e:
        idx.query_range_runs(t, k, 0, nw)
    assert e.value.code == _lib.KMHG_EOVERFLOW
    f = (1, 1, 46, 46, 1022, 1022)                   # 1,024 bins asked over 1..47000
    got, h = idx.raster(t, k, f)
    assert h == nw * nw == 2_207_684_196 and h > 2**31
    ci = raster_ref.window_counts(n, 1, 46, 1022) - raster_ref.window_counts(k - 1, 1, 46, 1022)
    cj = raster_ref.window_counts(nw, 1, 46, 1022)
    want = np.outer(ci, cj)
    assert int(want.sum()) == h
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------ 7. refusals
WORDS = ["null argument", "bin widths must be positive integers",
         "bin counts must be positive integers", "a raster has at most 2^26 cells",
         "the frame must lie within 1..2^31-1 on both axes"]


def test_refusals_their_words_and_order(gpu):
    torch = gpu
    from kmer_hasher_amd import _lib, device, synth
    from kmer_hasher_amd.device import DeviceIndex
    L = _lib.lib()
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    rows = _dev(torch, [(1, 1), (2, 2)])

    def refuse(frame, code=_lib.KMHG_EINVAL, rows_ptr=rows.data_ptr(), n=2, out_ptr=out.data_ptr()):
        fr = (C.c_int64 * 6)(*frame) if frame is not None else None
        rc = L.kmhg_rows_raster(C.c_void_p(rows_ptr), n, fr, C.c_void_p(out_ptr), None)
        assert rc == code
        return L.kmhg_last_error().decode()

    # each refusal, with every later fault present too: the earlier word wins
    assert refuse(None) == WORDS[0]
    assert refuse((0, 0, 0, 1, 0, 2**30), out_ptr=None) == WORDS[0]
    assert refuse((0, 0, 0, 1, 0, 2**30)) == WORDS[1]
    assert refuse((0, 0, 1, -3, 0, 2**30)) == WORDS[1]
    assert refuse((0, 0, 1, 1, 0, 2**30)) == WORDS[2]
    assert refuse((0, 0, 1, 1, 2**30, -1)) == WORDS[2]
    assert refuse((0, 0, 1, 1, 2**13, 2**13 + 1)) == WORDS[3]
    assert refuse((0, 0, 2**40, 1, 2**62, 2**62)) == WORDS[3]
    assert refuse((0, 1, 1, 1, 4, 4)) == WORDS[4]
    assert refuse((1, 0, 1, 1, 4, 4)) == WORDS[4]
    assert refuse((M, 1, 1, 1, 2, 1)) == WORDS[4]
    assert refuse((1, 2, 1, M, 1, 1)) == WORDS[4]
    assert refuse((1, 1, 2**31, 1, 1, 1)) == WORDS[4]
    assert refuse((1, 1, 2**40, 2**40, 4, 4), n=-1) == WORDS[4]
    assert refuse((1, 1, 1, 1, 4, 4), n=-1) == "bad row count"
    assert refuse((1, 1, 1, 1, 4, 4), n=2**31) == "bad row count"
    assert refuse((1, 1, 1, 1, 4, 4), rows_ptr=None) == WORDS[0]
    # the edge frames are legal, and n_rows = 0 reads no rows
    assert _rows_raster(torch, rows, (M, M, 1, 1, 1, 1)).tolist() == [[0]]
    assert _rows_raster(torch, rows, (1, 1, M, M, 1, 1)).tolist() == [[2]]
    assert int(device.rows_raster(rows, (1, 1, 1, 1, 2**13, 2**13)).sum()) == 2   # 2^26 cells
    fr = (C.c_int64 * 6)(1, 1, 1, 1, 4, 4)
    out.fill_(-1)
    _lib.check(L.kmhg_rows_raster(None, 0, fr, C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0

    # the query entries' refusals, in their words
    s = synth.iid(5000, 9)
    t = torch.from_numpy(s).cuda()
    idx = DeviceIndex.build(t, 31)
    f = (1, 1, 5, 5, 1000, 1000)
    ERR = "the sequence should be longer than k and k should not be longer than 31"
    for seq, k in ((t, 32), (t, 0), (t[:31], 31)):
        with pytest.raises(_lib.KmhgError) as e:
            idx.raster(seq, k, f)
        assert e.value.code == _lib.KMHG_EINVAL and str(e.value).endswith(ERR)
    with pytest.raises(_lib.KmhgError, match="bin widths must be positive"):
        idx.raster(t, 32, (1, 1, 0, 1, 4, 4))       # the frame is looked at before the query
    part = DeviceIndex.build_part(t, 31, 0, 2)
    with pytest.raises(_lib.KmhgError, match="a part index must be assembled before it is queried"):
        part.raster(t, 31, f)
    from kmer_hasher_amd import api
    sh = api.count_kmers_fq_sh_rp("no-such-file.fq", [15, 10, 0, 1, -1, 1, 1, 0])   # a counts index
    cells = torch.zeros(10**6, dtype=torch.int32, device="cuda")
    assert L.kmhg_raster_run_device(sh.handle, C.c_void_p(t.data_ptr()), t.numel(), 15, 0,
                                    (C.c_int64 * 6)(*f), C.c_void_p(cells.data_ptr()), None,
                                    None) == _lib.KMHG_EINVAL      # (sh keeps its handle)
    assert L.kmhg_last_error().decode() == "External pointer has incorrect tag"
    sh.free()
    # a handle that holds runs
    q, h, nr = C.c_void_p(), C.c_int64(), C.c_int64()
    _lib.check(L.kmhg_query_run_device_range_runs(
        idx.handle, C.c_void_p(t.data_ptr()), t.numel(), 31, 0, t.numel() - 30, None,
        C.byref(q), C.byref(h), C.byref(nr)))
    assert nr.value >= 0                             # it holds runs
    big = torch.zeros(10**6, dtype=torch.int32, device="cuda")
    fr = (C.c_int64 * 6)(*f)
    assert L.kmhg_query_raster(q, fr, C.c_void_p(big.data_ptr()), None) == _lib.KMHG_EINVAL
    assert L.kmhg_last_error().decode() == "the query holds runs (kmhg_query_runs_device)"
    L.kmhg_query_free(q)
    # and the library goes on
    got, n = idx.raster(t, 31, f)
    # row (i, j) of a self query has i = j + k - 1: bi = bj + 6 at bins of 5
    assert n == 4970 and int(got.sum()) == 4970 and int(torch.diagonal(got, -6).sum()) == 4970


def test_host_api(gpu, testfa):
    """seq_kmer_raster: default ranges, the bin rule, a pair of bins, ranges, rc."""
    from kmer_hasher_amd import api
    s = testfa[:3000]
    ptr = api.make_kmer_hash(s, 15)
    ox = O.OracleIndex(s, 15)
    fwd = ox.query(s, 15).reshape(-1, 2)
    r = api.seq_kmer_raster(ptr, s, 15, bins=1024)
    assert (r["i0"], r["j0"], r["bin_i"], r["bin_j"]) == (1, 1, 3, 3) and r["n_rows"] == len(fwd)
    assert r["counts"].dtype == np.int64 and r["counts"].shape == (1000, 1000)
    assert np.array_equal(r["counts"], raster_ref.raster(fwd, (1, 1, 3, 3, 1000, 1000)))
    r = api.seq_kmer_raster(ptr, s, 15, bins=(7, 300), i_range=(100, 2000), j_range=(5, 2999))
    assert (r["bin_i"], r["bin_j"], r["counts"].shape) == (272, 10, (7, 300))
    assert np.array_equal(r["counts"], raster_ref.raster(fwd, (100, 5, 272, 10, 7, 300)))
    rev = ox.query(rc_host(s), 15).reshape(-1, 2)
    r = api.seq_kmer_raster(ptr, s, 15, bins=100, rc=True)
    assert r["n_rows"] == len(rev)
    assert np.array_equal(r["counts"], raster_ref.raster(rev, (1, 1, 30, 30, 100, 100)))
    for kw, word in [(dict(bins=0), "bins should be"), (dict(bins=(1, 2, 3)), "bins should be"),
                     (dict(i_range=(0, 5)), "i.range should be"),
                     (dict(j_range=(9, 3)), "j.range should be"),
                     (dict(bins=(2**14, 2**14), i_range=(1, 2**20), j_range=(1, 2**20)),
                      "at most 2\\^26 cells")]:
        with pytest.raises(api.KmerHashError, match=word):
            api.seq_kmer_raster(ptr, s, 15, **kw)
    with pytest.raises(api.KmerHashError, match="should be longer than k"):
        api.seq_kmer_raster(ptr, "ACGT", 15)
    ptr.free()
